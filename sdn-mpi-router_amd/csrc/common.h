// common.h -- shared device helpers and the context layout of libsdnroute.
// gfx950 (CDNA4) only: 64-lane wavefronts, 160 KiB LDS per CU, 256 CUs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/sdnroute.h"

#define SDNR_WAVE 64
#define SDNR_LDS_PER_CU (160 * 1024)
#define SDNR_MAX_LDS_PER_BLOCK (160 * 1024)

// ---------------------------------------------------------------- device --

__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }

// number of set bits of m strictly below this lane
__device__ __forceinline__ int lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                          __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ int uniform(int x) {
    return __builtin_amdgcn_readfirstlane(x);
}

__device__ __forceinline__ int read_lane(int x, int lane) {
    return __builtin_amdgcn_readlane(x, lane);
}

__device__ __forceinline__ int highest_lane(uint64_t m) { return 63 - __clzll(m); }

// LDS bank swizzle for per-vertex u32 arrays indexed by neighbour ids: rows of
// structured fabrics hold strided ids (a fat-tree core's neighbours are 24
// apart: 8-way bank conflicts); x ^ ((x >> 3) & 31) is a bijection inside
// every 256-entry block and spreads those rows over all 32 banks.  Arrays
// indexed this way are sized in whole 256-entry blocks.
__device__ __forceinline__ int lds_swz(int x) { return x ^ ((x >> 3) & 31); }

// tree / next-hop rows as sdnr_link_loads and sdnr_multicast_trees take them
struct LoadRows {
    const uint32_t *tree;     // [nrows][V]: int32 parents / next hops, port16 or slot words
    int layout;               // SDNR_TREE_INT32 / SDNR_TREE_PORT16 / SDNR_TREE_SLOT
    int to_root;              // rows are next-hop rows: the edge is v -> parent
};

// parent of v (-1: the root, an unreached vertex, or a word that names no
// vertex of the graph -- *bad then); *slot: position of v in the parent's CSR
// row (slot layout only)
__device__ __forceinline__ int load_parent(const LoadRows &t, size_t rb, int v, int V, int *slot,
                                           bool *bad)
{
    const uint32_t w = t.tree[rb + v];
    int p;
    *slot = -1;
    if (t.layout == SDNR_TREE_PORT16) {
        p = (int)(w & 0xFFFFu);
        if (p == 0xFFFF) return -1;
    } else if (t.layout == SDNR_TREE_SLOT) {
        if (w == 0xFFFFFFFFu) return -1;
        p = (int)(w & 0x3FFFFFFu);
        *slot = (int)(w >> 26);
    } else {
        p = (int)w;
        if (p < 0) return -1;
    }
    if (p == v) return -1;                        // the root of a source tree
    if (p >= V) {
        *bad = true;
        return -1;
    }
    return p;
}

// index of the CSR entry (u, x), -1 if u has no such link
__device__ __forceinline__ int edge_index(const int32_t *__restrict__ row_ptr,
                                          const int32_t *__restrict__ col, int u, int x)
{
    int lo = row_ptr[u], hi = row_ptr[u + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return (lo < row_ptr[u + 1] && col[lo] == x) ? lo : -1;
}

// ------------------------------------------------------------------ host --

constexpr int kLiveRing = 8;           // runs of folded launches whose published count is still told apart

// what dfs_async_kernel expands a twin-class quotient's records with (one
// device word block, so the kernel carries one pointer through its search):
// VR the graph's vertex count, the rest sdnr_ctx's q_cid .. q_port
struct sdnr_quot {
    int32_t VR;
    const uint32_t *cid, *info, *loff;
    const uint8_t *slot;
    const int32_t *qport;
};

struct sdnr_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    // graph (device)
    int32_t V = -1, E = 0, max_deg = 0;
    uint64_t deg2_sum = 0;              // sum of squared out-degrees (sdnr_lfa_tables' nn entries)
    int32_t max_indeg = 0x7FFFFFFF;     // maximum in-degree (set with adj16/radj16)
    int32_t W = 0;                      // ELL row width (0: CSR only)
    int32_t *row_ptr = nullptr, *col = nullptr, *port = nullptr;
    uint32_t *cost = nullptr;           // per-link costs in edge order (sdnr_graph_costs)
    bool has_cost = false;              // costs uploaded for this graph (E may be 0)
    int32_t *ell_col = nullptr, *ell_port = nullptr;
    uint16_t *ell16 = nullptr;          // ELL ids as u16 (low 16 bits when V > 65535), 0xFFFF pad
    uint32_t *ell_hi = nullptr;         // per row: the 17th id bit of each slot (65535 < V <= 131071)
    // dictionary rows for the split DFS (V <= 65535, rows of <= 8 slots):
    // row u = u + dict_off[p(u) * 8 + slot], p(u) = byte (u & 31) of block
    // tuple dict_bt[b(u)] (32 pattern bytes = 8 u32 words), b(u) = byte
    // u >> 5 of dict_bp (4 block ids per u32 word, dict_bpw words); dict_off
    // dict_P x 8 int32 offsets (padding slots: kDictPad)
    uint32_t *dict_bp = nullptr;
    uint32_t *dict_bt = nullptr;
    int32_t *dict_off = nullptr;
    int32_t dict_P = 0, dict_NB = 0, dict_bpw = 0;
    uint16_t *adj16 = nullptr;          // (V+1) rows x 64 u16, sentinel V (V < 65535)
    uint16_t *radj16 = nullptr;         // in-neighbour rows, same layout (== adj16 if symmetric)
    uint32_t *deg32 = nullptr;          // out-degrees of 0..V (sentinel V: 0)
    uint16_t *radjw = nullptr;          // radj16 as swizzled count indices (async DFS workers)
    uint16_t *radjc = nullptr;          // ... for the compact-LDS form (word << 1 | half)
    bool radj_owned = false;
    // in-degree <= 32: the pre-swizzled rows (radjw / radjc) repeat their 32
    // entries in lanes 32..63, so one 64-lane load + ds_sub covers 2 children
    bool radj_pair = false;
    // out-rows as arithmetic runs (dfs_runs.hip): (V+1) rows x runs_R words
    // of start | stride << 16 | count << 25
    uint32_t *runs = nullptr;
    int32_t runs_R = 0;
    // bitmap rows for the register-visited DFS (dfs_bits.hip, V <= 4096):
    // adjb[u * 64 + l] = bits of u's out-neighbours 64l..64l+63, adjp the
    // exclusive prefix popcount of lane blocks (u8), radjx[v * 64 + i] =
    // swizzled count index | in-neighbour << 16 (padding: dummy | 0xFFFF << 16;
    // row V all padding)
    uint64_t *adjb = nullptr;
    uint8_t *adjp = nullptr;
    uint32_t *radjx = nullptr;
    // twin classes: twin_rep[v] = smallest vertex with v's
    // out-row and in-row (v itself when its row holds a self-loop); the DFS
    // rows of a class differ in 2 + |row| entries, so a batch searches one
    // member per class and derives the others (sdnr_launch_dfs)
    int32_t *twin_rep = nullptr;
    bool has_twins = false;             // some class has more than one member
    // the twin-class quotient (built with the u16 rows of a
    // graph with twins): its vertices are the classes, numbered by ascending
    // largest member, and dfs_async_kernel searches it in place of the graph.
    // q_adj16 .. q_radjc are the quotient's rows in the layouts of adj16 ..
    // radjc (paired exactly when the graph's are); q_cid[v] = class of v |
    // rank of v in its class << 16; q_info[c] = largest member | (more than
    // one member) << 16; q_slot[q_loff[c * 64 + j] + r] = the slot, in the
    // out-row of c's members, of the member of rank r of the class in slot j
    // of c's quotient row, and q_port[the same index] that link's port -- the
    // slot table composed with the port row of c's largest member, so the
    // flush takes a tree link's port in one gather
    int32_t q_V = 0, q_E = 0;
    uint16_t *q_adj16 = nullptr, *q_radj16 = nullptr, *q_radjw = nullptr, *q_radjc = nullptr;
    uint32_t *q_deg32 = nullptr;
    bool q_radj_owned = false;
    uint32_t *q_cid = nullptr, *q_info = nullptr, *q_loff = nullptr;
    uint8_t *q_slot = nullptr;
    int32_t *q_port = nullptr;
    struct sdnr_quot *q_tab = nullptr;  // the expansion tables as the kernel takes them (device)
    bool dfs_quotient = false;          // the last DFS launch searched the quotient
    // the last DFS launch on this context: its batch size, and whether it
    // folded (then the searched count is the int at the head of scratch3)
    int32_t dfs_nsrc = 0;
    bool dfs_folded = false;
    int32_t dfs_form = 0;               // kDfsFormFull / kDfsFormLow of that launch's search
    // the fold's live count as a hint for the next folded call (dfs.hip,
    // DESIGN.md 4.1e): dfs_fold_derive_kernel stores sequence << 32 | count
    // into h_live, a coherent mapped host word; the host reads it without
    // waiting, and live_ring tells which launch a sequence number was: an
    // entry is a run seq0..seq1 of consecutive folded launches of one upload
    // and batch size (the host may be any number of equal calls ahead of the
    // device).  Per context, so every peer and every stream's context has its own
    unsigned long long *h_live = nullptr;
    struct {
        uint32_t seq0, seq1, gen;       // seq0 0: no launch
        int32_t nsrc;
    } live_ring[kLiveRing] = {};
    int live_head = 0;                  // the newest run
    uint32_t live_seq = 0;              // the last folded launch's sequence number
    uint32_t upload_gen = 0;            // bumped by every graph upload (free_graph)

    // grow-only device scratch / staging
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    void *stage = nullptr;
    size_t stage_bytes = 0;
    void *scratch2 = nullptr;           // int32 tables behind a packed-table call
    size_t scratch2_bytes = 0;
    void *scratch3 = nullptr;           // the twin fold's lists and leader tables (dfs.hip)
    size_t scratch3_bytes = 0;
    void *wq = nullptr;                 // source work queue of the split DFS (kFlagCuMap)
    size_t wq_bytes = 0;
    void *dmat = nullptr;               // V x V distances behind APSP-derived shortest tables
    size_t dmat_bytes = 0;
    // the route expansion's walk tables (packed trees + u16 ancestor tables)
    // and what they were built from (SDNR_SAME_TABLES reuses them)
    void *anc = nullptr;
    size_t anc_bytes = 0;
    const void *anc_parent = nullptr, *anc_port = nullptr;
    size_t anc_n = 0;
    bool anc_valid = false;
    bool port16 = false;                // every port fits the packed layout (< 0xFFFF)
    bool symmetric = false;             // every link (u, v) has its reverse (v, u)

    // timing of the main kernel(s) of the last SDNR_TIMING call
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    const char *last_kernel = "";       // variant launched by the last table call
    int32_t last_launches = 0;          // main-kernel launches of the last table call
    int64_t last_grid = 0;              // workgroups of the last row-persistent launch (sdnr_last_grid)
    int32_t last_sweeps = 0;            // Bellman-Ford sweeps of the last APSP call
    int32_t plane_depth = 0;            // levels the bit-plane BFS last needed on this graph
    // sdnr_frr_link_loads: the affected-item count of the last call, copied
    // into a pinned host word behind its kernels (sdnr_last_frr_items)
    int64_t *h_frr_items = nullptr;
    bool frr_items_pending = false;     // the last call launched: the word is (or will be) its count
    int *d_err = nullptr;               // kernel watchdog word (0 = ok)
    int *h_flag = nullptr;              // pinned host words for level-loop checks
    int *h_pub = nullptr;               // coherent host words a kernel publishes into
    int pub_seq = 0;                    // sequence number of the last publication
    hipEvent_t ev_flag = nullptr;       // ... and the event the host spins on

    // multi-device context (sdnr_create_multi): this context is shard 0 on
    // the primary device; peers[k] own shard k+1 (own device, stream, graph
    // copy and scratch).  fork/join events order the peers' streams after /
    // before the primary stream.
    sdnr_ctx **peers = nullptr;
    int npeers = 0;
    hipEvent_t ev_fork = nullptr;       // recorded on the primary stream
    hipEvent_t ev_join = nullptr;       // per context: recorded on its own stream
};

// Raise a kernel's dynamic-LDS limit; a refusal (e.g. static LDS + bytes >
// 160 KiB) is cleared so it cannot surface later as hipGetLastError().
inline void sdnr_allow_lds(const void *fn, size_t bytes)
{
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
        hipSuccess)
        (void)hipGetLastError();
}

// watchdog-word codes a kernel ORs into ctx->d_err (dfs.hip uses 1..16 for
// bounded waits that ran out, and 32 for the split kernel's CU-numbering spin,
// split_cu_number); sdnr_synchronize turns a nonzero word into an error, the
// specific INVAL causes below tested bit by bit (a word may hold several)
// A/B tuning knobs that only select non-default shapes (worker widths,
// block shapes, store hints): read by the diagnostic build alone
// (tools/diag/build_diag.sh, -DSDNR_DIAG_VARIANTS); the product library
// always takes its measured defaults (knob sprawl)
inline const char *sdnr_tune_env(const char *name)
{
#ifdef SDNR_DIAG_VARIANTS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

constexpr int kDfsFormFull = 0, kDfsFormLow = 1;   // sdnr_ctx::dfs_form (sdnr_last_dfs_form)
constexpr int kDictPad = 0x40000000;   // dictionary-row padding offset (u + pad >= V)
constexpr int kDictMaxP = 255;         // pattern ids are bytes
constexpr int kErrLastPort = 256;   // sdnr_route_expand_packed: a last port outside [0, 0xFFFE]
constexpr int kErrTreeClimb = 512;  // sdnr_dfs_rows_affected: a tree climb outran V steps
constexpr int kErrScan = 1024;      // sdnr_route_offsets: a look-back wait ran out
constexpr int kErrSeg = 2048;       // route expansion: a walker / storer hand-off wait ran out
constexpr int kErrLoadsTree = 4096; // sdnr_link_loads: a row is not a tree of the graph / bad offsets

// sdnr_link_loads keeps a row's sums and ancestors in LDS (20 bytes per
// vertex: 160,000 of the CU's 163,840) up to this V, else in global scratch
// (24 bytes per vertex and workgroup, at most kLoadsScratchBytes in all)
constexpr int kLoadsLdsMaxV = 8000;
constexpr size_t kLoadsScratchBytes = (size_t)1 << 30;
constexpr int kErrEcmpLoads = 8192; // sdnr_ecmp_link_loads: a dist row is no BFS labelling / bad offsets

// sdnr_ecmp_link_loads keeps a row's levels, route counts and flows in LDS
// (16 control bytes + 18 per vertex: 162,016 of the CU's 163,840) up to this V,
// else the counts and flows in global scratch (16 bytes per vertex and
// workgroup, at most kLoadsScratchBytes in all)
constexpr int kEcmpLoadsLdsMaxV = 9000;
constexpr int kErrCostTables = 16384; // sdnr_cost_tables: V sweeps did not reach the fixed point

// sdnr_cost_tables keeps the least-cost rows of a batch of destinations in
// LDS: 8 of them (32 bytes per vertex) up to kCostLdsMaxV8 vertices, 4 (16
// bytes per vertex) up to kCostLdsMaxV -- 160,000 of the CU's 163,840 bytes at
// either cap --, else 4 in global scratch (16 bytes per vertex and workgroup,
// at most kLoadsScratchBytes in all)
constexpr int kCostLdsMaxV8 = 5000;
constexpr int kCostLdsMaxV = 10000;
constexpr int kErrCostEcmpLoads = 32768; // sdnr_cost_ecmp_link_loads: a pcost row is no least-cost labelling / bad offsets

// sdnr_cost_ecmp_link_loads keeps a row's route counts, flows, costs and
// depths in LDS (22 bytes per vertex) up to this V -- what the CU's LDS holds,
// rounded down to a hundred: 7,400, 162,800 of 163,840 bytes --,
// else the counts, flows and depths in global scratch (20 bytes per vertex and
// workgroup, at most kLoadsScratchBytes in all)
constexpr int kCostEcmpBytesPerV = 22;
constexpr int kCostEcmpLdsMaxV = SDNR_LDS_PER_CU / kCostEcmpBytesPerV / 100 * 100;
static_assert(kCostEcmpLdsMaxV == 7400 && kCostEcmpLdsMaxV < 0xFFFF, "depths in LDS are u16");
constexpr int kErrFailureLoads = 65536; // sdnr_failure_ecmp_link_loads: a bad failed-link list / bad offsets / sweeps past V

// sdnr_failure_ecmp_link_loads keeps a (scenario, row) item's route counts,
// flows, costs, depths and failed-link flags in LDS (23 bytes per vertex) up to
// this V -- what the CU's LDS holds, rounded down to a hundred: 7,100, 163,300
// of 163,840 bytes --, else all of them in global scratch (u32 depths: 25
// bytes per vertex and workgroup, at most kLoadsScratchBytes in all)
constexpr int kFailureBytesPerV = 23;
constexpr int kFailureLdsMaxV = SDNR_LDS_PER_CU / kFailureBytesPerV / 100 * 100;
static_assert(kFailureLdsMaxV == 7100 && kFailureLdsMaxV < 0xFFFF, "depths in LDS are u16");

constexpr int kErrLfa = 131072; // sdnr_lfa_tables: a row with P[d][d] != 0 / a vertex of finite cost > 0 without a tight link

// sdnr_lfa_tables reads an all-pairs [V][V] u32 table and keeps one row of it
// in LDS (64 KiB at the cap, sdnr_apsp's); its per-link and per-neighbour-pair
// pre-pass arrays live in the context scratch (at most kLoadsScratchBytes)
constexpr int kLfaMaxV = 16384;
constexpr int kErrWhatifLoads = 262144; // sdnr_whatif_ecmp_link_loads: a bad override list / bad offsets / sweeps past V / a bad capacity

constexpr int kErrWidest = 524288; // sdnr_widest_tables: a row with pcost[d] != 0 / a vertex of finite cost > 0 without a tight route / sweeps past V

// sdnr_widest_tables keeps pcost and bott of a batch of destinations in LDS:
// 6 of them (48 bytes per vertex) up to kWidestLdsMaxV6 vertices, 4 (32 bytes)
// up to kWidestLdsMaxV4, 2 (16 bytes) up to kWidestLdsMaxV -- 159,984 or
// 160,000 of the CU's 163,840 bytes at the caps --, else 4 in global scratch
// (32 bytes per vertex and workgroup, at most kLoadsScratchBytes in all)
constexpr int kWidestLdsMaxV6 = 3333;
constexpr int kWidestLdsMaxV4 = 5000;
constexpr int kWidestLdsMaxV = 10000;

constexpr int kErrFairRates = 1048576; // sdnr_fair_rates: a row is not a tree of the graph / bad offsets / a bad capacity or extra

// sdnr_fair_rates keeps a row's subtree sums, ancestors and link indices in
// LDS (two u64 and two u16 generations and one i32: 24 bytes per vertex; the
// first-saturated-link search aliases the sums) up to this V -- what the CU's
// LDS holds, rounded down to a hundred: 6,800, 163,200 of 163,840 bytes --,
// else in global scratch (u32 ancestors: 28 bytes per vertex and workgroup, at
// most kLoadsScratchBytes in all)
constexpr int kFairBytesPerV = 24;
constexpr int kFairLdsMaxV = SDNR_LDS_PER_CU / kFairBytesPerV / 100 * 100;
static_assert(kFairLdsMaxV == 6800 && kFairLdsMaxV < 0xFFFF, "ancestors in LDS are u16");

constexpr int kErrFairTimes = 16777216; // sdnr_fair_times: sdnr_fair_rates' row, offset, capacity and extra errors, or a byte size that is negative or not finite

constexpr int kErrEcmpFairRates = 2097152; // sdnr_ecmp_fair_rates: a pcost row is no least-cost labelling / bad offsets / a bad capacity or extra
constexpr int kErrEcmpFairTimes = 33554432; // sdnr_ecmp_fair_times: sdnr_ecmp_fair_rates' row, offset, capacity and extra errors, or a byte size that is negative or not finite

// sdnr_ecmp_fair_rates keeps a row's route counts, flows (the saturated-link
// search aliases them), costs and depths in LDS (f64 + f64 + u32 + u16: 22
// bytes per vertex, sdnr_cost_ecmp_link_loads' row state) up to this V -- what
// the CU's LDS holds beside the kernel's static words (the alive count and the
// barrier votes, under 512 bytes), rounded down to a hundred: 7,400, 162,800 of
// 163,840 bytes --, else the counts, flows and
// depths in global scratch (20 bytes per vertex and workgroup, at most
// kLoadsScratchBytes in all)
constexpr int kEcmpFairBytesPerV = 22;
constexpr int kEcmpFairLdsMaxV = SDNR_LDS_PER_CU / kEcmpFairBytesPerV / 100 * 100;
static_assert(kEcmpFairLdsMaxV == 7400 && kEcmpFairLdsMaxV < 0xFFFF, "depths in LDS are u16");
static_assert(kEcmpFairLdsMaxV * kEcmpFairBytesPerV + 16 + 512 <= SDNR_LDS_PER_CU,
              "the row state, its 16-byte rounding and the static words fit the CU's LDS");

constexpr int kErrMcast = 4194304; // sdnr_multicast_trees: a row is not a tree of the graph / bad offsets

// sdnr_multicast_trees keeps a group's visited map (V bits) and link map (E
// bits) in LDS while their u32 words fit kMcastLdsBytes -- 32 KiB, so four
// 256-thread workgroups share a CU's 160 KiB --, else in a per-workgroup slice
// of the context's scratch (global atomics; at most kLoadsScratchBytes in all)
constexpr size_t kMcastLdsBytes = 32 * 1024;
static_assert(4 * kMcastLdsBytes + 4 * 1024 <= SDNR_LDS_PER_CU,
              "four workgroups' maps and their static words fit the CU's LDS");

constexpr int kErrFrrLoads = 8388608; // sdnr_frr_link_loads: a row that is no in-tree / a next hop or backup that is no out-neighbour / a bad scenario list / bad offsets

// sdnr_frr_link_loads keeps an item's doubling generations (two u64, two u16),
// its classification word (u32) and its patched next hop (u16) in LDS: 26
// bytes per vertex, up to this V -- what the CU's LDS holds beside the kernel's
// static words (the barrier votes, under 512 bytes), rounded down to a hundred:
// 6,200, 161,200 of 163,840 bytes.  There is no global-scratch form.
constexpr int kFrrBytesPerV = 26;
constexpr int kFrrMaxV = (SDNR_LDS_PER_CU - 512) / kFrrBytesPerV / 100 * 100;
static_assert(kFrrMaxV == 6200 && kFrrMaxV < 0xFFFF, "next hops in LDS are u16");

// error plumbing (capi.hip)
int sdnr_fail(int code, const char *fmt, ...);
int sdnr_hip_fail(hipError_t e, const char *what);
int sdnr_reserve(void **buf, size_t *cur, size_t need);
int sdnr_check_watchdog(sdnr_ctx *ctx);   // after a stream sync
// copy n (<= 4) ints from the device into out and wait for them with a
// busy spin on an event: a level loop's termination check costs a few
// microseconds instead of a blocking stream synchronize's wake-up
int sdnr_fetch_ints(sdnr_ctx *ctx, const int *d_src, int n, int *out);
// the same in two halves: the copy + event go on the stream, more work may
// follow them, then the host waits for the event (the words as of then)
int sdnr_wait_published(sdnr_ctx *ctx, int seq, int n, int *out);

#define SDNR_HIP(call)                                           \
    do {                                                         \
        hipError_t _e = (call);                                  \
        if (_e != hipSuccess) return sdnr_hip_fail(_e, #call);   \
    } while (0)

// kernel launchers (dfs.hip, shortest.hip, apsp.hip); device pointers,
// asynchronous on ctx->stream
int sdnr_launch_dfs(sdnr_ctx *ctx, const int32_t *d_src, int32_t nsrc,
                    int32_t *d_parent, int32_t *d_port, int32_t *d_hops,
                    uint32_t *d_tree,         // d_tree: packed layout instead of the three
                    bool slots = false,       // d_tree as parent | slot << 26
                    bool hops16 = false);     // d_hops as u16 (0xFFFF unreached)
// int32 trees -> parent | port << 16 or parent | slot << 26 (dfs.hip)
int sdnr_launch_tree_pack(sdnr_ctx *ctx, const int32_t *parent, const int32_t *port, size_t n,
                          uint32_t *tree, bool slots);
#ifdef SDNR_DIAG_VARIANTS
// the diagnostic build's losing DFS variants (tools/diag/)
// register-visited DFS (dfs_bits.hip): V <= 4096 with bitmap rows uploaded
bool sdnr_dfs_bits_ok(const sdnr_ctx *ctx);
int sdnr_launch_dfs_bits(sdnr_ctx *ctx, const int32_t *d_src, int32_t nsrc, int32_t *d_parent,
                         int32_t *d_port, int32_t *d_hops, uint32_t *d_tree, bool hops16);
// LDS-row DFS (dfs_runs.hip): usable when the run-encoded rows plus one
// source's state fit a workgroup's LDS
bool sdnr_dfs_runs_ok(const sdnr_ctx *ctx, bool hops);
int sdnr_launch_dfs_runs(sdnr_ctx *ctx, const int32_t *d_src, int32_t nsrc, int32_t *d_parent,
                         int32_t *d_port, int32_t *d_hops, uint32_t *d_tree);
#endif
int sdnr_launch_shortest(sdnr_ctx *ctx, const int32_t *d_dst, int32_t ndst,
                         uint16_t *d_dist, int32_t *d_nh, int32_t *d_nh_port);
int sdnr_launch_apsp(sdnr_ctx *ctx, uint16_t *d_dist);
int sdnr_launch_ecmp_counts(sdnr_ctx *ctx, const uint16_t *d_dist, int32_t ndst,
                            uint64_t *d_paths);
int sdnr_launch_ecmp_unrank(sdnr_ctx *ctx, const uint16_t *d_dist, const uint64_t *d_paths,
                            const int32_t *d_rows, const int32_t *d_srcs, const uint64_t *d_ranks,
                            int32_t nroutes, int32_t max_len, int32_t *d_out);
int sdnr_launch_route_offsets(sdnr_ctx *ctx, const int32_t *d_hops, const int32_t *d_rows,
                              const int32_t *d_dsts, int32_t npairs, int64_t *d_off);
int sdnr_launch_route_expand(sdnr_ctx *ctx, const int32_t *d_parent, const int32_t *d_port,
                             int32_t nrows, const int32_t *d_rows, const int32_t *d_dsts,
                             const int32_t *d_last_port, int32_t npairs, const int64_t *d_off,
                             int32_t *d_switch, int32_t *d_hport, uint32_t *d_entries = nullptr,
                             bool same_tables = false);
// rows of cached default-route trees a link change alters (incremental.hip)
int sdnr_launch_dfs_rows_affected(sdnr_ctx *ctx, const uint32_t *d_tree, const void *d_depth,
                                  int32_t layout, int32_t depth_bytes, int32_t nrows,
                                  const int32_t *d_row_src, const int32_t *d_links, int32_t nrm,
                                  int32_t nadd, uint8_t *d_affected);
// per-link loads of a demand routed over tree rows (loads.hip); pair_lo /
// pair_hi = pair_off[0] / pair_off[nrows], the bounds of the pair list
int sdnr_launch_link_loads(sdnr_ctx *ctx, const void *d_tree, int32_t layout, bool to_root,
                           int32_t nrows, const int64_t *d_pair_off, int64_t pair_lo,
                           int64_t pair_hi, const int32_t *d_dsts, const uint64_t *d_weight,
                           uint64_t *d_load);
// per-link loads of a demand split over every shortest route (ecmp_loads.hip)
int sdnr_launch_ecmp_link_loads(sdnr_ctx *ctx, const uint16_t *d_dist, int32_t nrows,
                                const int64_t *d_pair_off, int64_t pair_lo, int64_t pair_hi,
                                const int32_t *d_srcs, const uint64_t *d_weight, double *d_load,
                                bool hop);
// least-cost tables under the uploaded per-link costs (cost_tables.hip)
int sdnr_launch_cost_tables(sdnr_ctx *ctx, const int32_t *d_dst, int32_t ndst, uint32_t *d_pcost,
                            int32_t *d_nh, int32_t *d_nh_port);
// per-link loads of a demand split over every least-cost route (cost_ecmp_loads.hip)
int sdnr_launch_cost_ecmp_link_loads(sdnr_ctx *ctx, const uint32_t *d_pcost, int32_t nrows,
                                     const int64_t *d_pair_off, int64_t pair_lo, int64_t pair_hi,
                                     const int32_t *d_srcs, const uint64_t *d_weight,
                                     double *d_load, bool hop);
// ... once per failure scenario, the scenario's links masked out (failure_loads.hip);
// scen_lo / scen_hi = scen_off[0] / scen_off[nscen]
int sdnr_launch_failure_ecmp_link_loads(sdnr_ctx *ctx, const int32_t *d_dst, int32_t nrows,
                                        const int64_t *d_pair_off, int64_t pair_lo,
                                        int64_t pair_hi, const int32_t *d_srcs,
                                        const uint64_t *d_weight, int32_t nscen,
                                        const int64_t *d_scen_off, int64_t scen_lo,
                                        int64_t scen_hi, const int32_t *d_scen_edges,
                                        double *d_load, double *d_lost, uint8_t *d_routed,
                                        bool hop);
// ... once per cost scenario, the scenario's cost overrides in force (whatif_loads.hip),
// and the peak utilisation of every [E] slice of a load plane
int sdnr_launch_whatif_ecmp_link_loads(sdnr_ctx *ctx, const int32_t *d_dst, int32_t nrows,
                                       const int64_t *d_pair_off, int64_t pair_lo,
                                       int64_t pair_hi, const int32_t *d_srcs,
                                       const uint64_t *d_weight, int32_t nscen,
                                       const int64_t *d_scen_off, int64_t scen_lo,
                                       int64_t scen_hi, const int32_t *d_scen_edges,
                                       const uint32_t *d_scen_costs, double *d_load,
                                       double *d_lost, uint8_t *d_routed, bool hop);
// fast-reroute what-if loads: LFA repair active, per failure scenario (frr_loads.hip),
// and the largest entry of every [E] slice of a u64 load plane
int sdnr_launch_frr_link_loads(sdnr_ctx *ctx, const int32_t *d_dst, const int32_t *d_nh,
                               const int32_t *d_backup, int32_t nrows, const int64_t *d_pair_off,
                               int64_t pair_lo, int64_t pair_hi, const int32_t *d_srcs,
                               const uint64_t *d_weight, int32_t nscen,
                               const int64_t *d_scen_off, int64_t scen_lo, int64_t scen_hi,
                               const int32_t *d_scen_edges, uint64_t *d_load, uint64_t *d_stat,
                               uint8_t *d_status);
int sdnr_launch_frr_peak(sdnr_ctx *ctx, int32_t nscen, const uint64_t *d_load, uint64_t *d_peak,
                         int32_t *d_peak_edge);
int sdnr_launch_whatif_peak(sdnr_ctx *ctx, int32_t nscen, const double *d_load,
                            const double *d_capacity, double *d_peak, int32_t *d_peak_edge);
// loop-free alternate next hops per destination (lfa_tables.hip)
int sdnr_launch_lfa_tables(sdnr_ctx *ctx, const uint32_t *d_pcost_all, const int32_t *d_dst,
                           int32_t ndst, int32_t *d_backup, int32_t *d_backup_port,
                           uint8_t *d_kind, uint32_t *d_counts, bool link_only);
// remote loop-free alternates: a PQ-node repair tunnel per link (remote_lfa.hip)
int sdnr_launch_remote_lfa(sdnr_ctx *ctx, const uint32_t *d_pcost_all, const int32_t *d_verts,
                           int32_t nverts, int32_t *d_pq, int32_t *d_via, int32_t *d_via_port,
                           uint64_t *d_tunnel_cost, uint8_t *d_kind, uint32_t *d_counts);
// least-loaded (min-max utilisation) next hops inside the least-cost DAG (widest_tables.hip)
int sdnr_launch_widest_tables(sdnr_ctx *ctx, const uint32_t *d_pcost, const uint32_t *d_util,
                              const int32_t *d_dst, int32_t ndst, uint32_t *d_bott, int32_t *d_nh,
                              int32_t *d_nh_port);
// max-min fair rates of flows routed over tree rows (fair_rates.hip); waits for
// the rounds and writes *nrounds
int sdnr_launch_fair_rates(sdnr_ctx *ctx, const void *d_tree, int32_t layout, bool to_root,
                           int32_t nrows, const int64_t *d_pair_off, int64_t pair_lo,
                           int64_t pair_hi, const int32_t *d_verts, const uint64_t *d_mult,
                           const int32_t *d_extra, const double *d_cap, int32_t nextra,
                           double *d_rate, int32_t *d_bott, int32_t *d_round, double *d_level,
                           int32_t max_rounds, double *d_used, int32_t *nrounds);
// max-min fair completion times of flows routed over tree rows
// (fair_times.hip); waits for the epochs and writes *nepochs
int sdnr_launch_fair_times(sdnr_ctx *ctx, const void *d_tree, int32_t layout, bool to_root,
                           int32_t nrows, const int64_t *d_pair_off, int64_t pair_lo,
                           int64_t pair_hi, const int32_t *d_verts, const uint64_t *d_mult,
                           const double *d_bytes, const int32_t *d_extra, const double *d_cap,
                           int32_t nextra, double *d_time, int32_t *d_epoch, double *d_rate0,
                           double *d_remaining, double *d_epoch_time, int32_t *d_epoch_rounds,
                           int32_t max_epochs, double *d_carried, int32_t *nepochs);
// max-min fair rates of flows split over every least-cost route
// (ecmp_fair_rates.hip); waits for the rounds and writes *nrounds
int sdnr_launch_ecmp_fair_rates(sdnr_ctx *ctx, const uint32_t *d_pcost, int32_t nrows,
                                const int64_t *d_pair_off, int64_t pair_lo, int64_t pair_hi,
                                const int32_t *d_srcs, const uint64_t *d_mult,
                                const int32_t *d_extra, const double *d_cap, int32_t nextra,
                                double *d_rate, int32_t *d_bott, int32_t *d_round, double *d_level,
                                int32_t max_rounds, double *d_used, int32_t *nrounds, bool hop);
// max-min fair completion times of flows split over every least-cost route
// (ecmp_fair_times.hip); waits for the epochs and writes *nepochs
int sdnr_launch_ecmp_fair_times(sdnr_ctx *ctx, const uint32_t *d_pcost, int32_t nrows,
                                const int64_t *d_pair_off, int64_t pair_lo, int64_t pair_hi,
                                const int32_t *d_srcs, const uint64_t *d_mult,
                                const double *d_bytes, const int32_t *d_extra, const double *d_cap,
                                int32_t nextra, double *d_time, int32_t *d_epoch, double *d_rate0,
                                double *d_remaining, double *d_epoch_time,
                                int32_t *d_epoch_rounds, int32_t max_epochs, double *d_carried,
                                int32_t *nepochs, bool hop);
// multicast trees of groups of members over tree / next-hop rows (multicast.hip);
// mem_lo / mem_hi = mem_off[0] / mem_off[ngroups], ent_lo / ent_hi likewise of ent_off
int sdnr_launch_multicast_trees(sdnr_ctx *ctx, const void *d_tree, int32_t layout, bool to_root,
                                int32_t nrows, int32_t ngroups, const int32_t *d_root,
                                const int64_t *d_mem_off, int64_t mem_lo, int64_t mem_hi,
                                const int32_t *d_mem_row, const int32_t *d_mem_vertex,
                                const uint64_t *d_weight, uint8_t *d_reached, int64_t *d_ent_cnt,
                                const int64_t *d_ent_off, int64_t ent_lo, int64_t ent_hi,
                                int32_t *d_ent_edge, uint64_t *d_load);
int sdnr_launch_edge_ports(sdnr_ctx *ctx, const uint64_t *d_ends, int32_t nends,
                           const uint64_t *d_ports, int32_t nports, uint8_t *d_is_edge);
