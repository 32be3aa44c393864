// fair_rates.hip -- max-min fair flow rates over single-path route tables.
//
// A link load says how much crosses a link; what a rank pair gets follows from
// the loads only through a sharing rule.  Flows on a fabric (TCP, RoCE with
// DCQCN) share bandwidth approximately max-min fairly, and the max-min fair
// allocation is unique: progressive filling finds it.  A flow is a pair of
// sdnr_link_loads (table row r, vertex x) with a multiplicity and up to two
// extra constraints (host ports); its links are the tree links from x to the
// row's root.  With rem = cap, used = 0, n_prev = 0, round k = 0, 1, ...:
//   1. n[e]  = sum of mult over the alive flows crossing e (u64, exact);
//   2. k > 0: m = n_prev[e] - n[e], p = r_{k-1} * (double)m, used[e] += p,
//      rem[e] = max(rem[e] - p, 0)            (each operation rounded alone);
//   3. share[e] = rem[e] / n[e] (n[e] > 0, else +inf), r_k = min share;
//      r_k = +inf: nothing alive crosses anything, stop;
//   4. e is saturated iff share[e] == r_k; every alive flow crossing a
//      saturated link or constraint gets rate r_k, round k and bott = the
//      first saturated tree link from x toward the root, else extra 0, else
//      extra 1, and is dead; n_prev = n.
// Every operation is deterministic (u64 counts, one double operation per link
// and round, a minimum), so the host restatement (engine.fair_rates_host)
// agrees bit for bit.
//
// No grid-wide barrier and no waiting between workgroups: a round is two plain
// launches on the context's stream.
//   fair_rows_kernel (round k), one workgroup per row, persistent over rows:
//     the verdict of round k - 1 and the counts of round k share ONE launch --
//     the verdict only reads share[] / level[k-1] (written by the link kernel
//     before it) and the counts only add into n[] (zeroed by it).
//     Per row visit e_v (the link of v toward the root) is looked up once.
//     (a) verdict: B_0[v] = share[e_v] == r_{k-1} ? e_v : none, J_0 = parent,
//         B_{j+1}[v] = B_j[v] != none ? B_j[v] : B_j[J_j[v]], J_{j+1} = J_j o J_j
//         (gathers only); the row's alive flows read B[x] and their extras'
//         shares and store rate, round, bott.
//     (b) counts: A_0[v] = alive multiplicity at v, subtree sums by the
//         ancestor doubling of loads.hip, one u64 atomic per vertex with a
//         nonzero sum into n[e_v] and one per alive flow's extra.
//     Round 0 classifies the flows instead of (a).  A per-row alive counter
//     lets a row with no alive flow return at once.  Both doublings take
//     ceil(log2(depth + 1)) steps and are bounded by ceil(log2 V) + 1: a row
//     that is no tree sets the error bit, its flows read 0.0 / -1 / -1 and it
//     contributes nothing.  A (two u64 generations), J (two generations, u16)
//     and e_v (i32) live in LDS, 24 bytes per vertex, up to kFairLdsMaxV; B
//     (two i32 generations) aliases A, which (b) fills only after (a) is done.
//     Above that they live in a per-workgroup slice of the context's scratch
//     (u32 ancestors, 28 bytes per vertex), as in loads.hip.
//   fair_links_kernel (round k), over the E + nextra entries: step 2, share,
//     n_prev = n, n = 0, a wave-reduced minimum into level[k] (atomicMin on the
//     bits: non-negative doubles order as their bit patterns), and the last
//     workgroup to finish stores k + 1 into the status word if level[k] is
//     +inf.  A kernel launched after that sees the status and returns.
// The host queues kFairBatch rounds, reads the 8-byte status word back, and
// goes on until it is set (or max_rounds rounds were run).
#include "common.h"

#include <string.h>

namespace {

constexpr int kFairThreads = 512;
constexpr int kFairLinkThreads = 256;
constexpr int kFairBatch = 16;           // rounds queued per status read-back
constexpr int kFairAlive = -2;           // round[] of a flow not frozen yet
constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;

struct FairRows {
    const uint32_t *tree;     // [nrows][V]: int32 parents / next hops, port16 or slot words
    int layout;               // SDNR_TREE_INT32 / SDNR_TREE_PORT16 / SDNR_TREE_SLOT
    int to_root;              // rows are next-hop rows: the link is v -> parent
};

struct FairState {
    unsigned long long *n;        // [E + nextra] counts of the running round (zero between rounds)
    unsigned long long *n_prev;   // [E + nextra] counts of the round before
    double *rem;                  // [E + nextra] capacity left
    double *share;                // [E + nextra] rem / n of the last link pass
    double *used;                 // [E + nextra] the caller's
    unsigned long long *level;    // [max_rounds + 1] bits of r_k, +inf until round k ran
    long long *alive_row;         // [nrows] alive flows of a row
    unsigned long long *status;   // 0: running, k + 1: r_k was +inf
    unsigned int *ticket;         // workgroups of the running link pass that are done
};

// what the tree word of v says: its parent (kFairNone: none), and whether v is
// a root of the row (its own parent, or -- in next-hop rows, which hold -1 at
// the destination -- without a next hop)
constexpr int kFairNone = -1, kFairBadWord = -2;

__device__ __forceinline__ int fair_parent(const FairRows &t, size_t rb, int v, int V, int *slot,
                                           bool *root)
{
    const uint32_t w = t.tree[rb + v];
    int p;
    *slot = -1;
    *root = false;
    if (t.layout == SDNR_TREE_PORT16) {
        p = (int)(w & 0xFFFFu);
        if (p == 0xFFFF) return kFairNone;
    } else if (t.layout == SDNR_TREE_SLOT) {
        if (w == 0xFFFFFFFFu) return kFairNone;
        p = (int)(w & 0x3FFFFFFu);
        *slot = (int)(w >> 26);
    } else {
        p = (int)w;
        if (p < 0) {
            *root = t.to_root != 0;
            return kFairNone;
        }
    }
    if (p == v) {
        *root = true;
        return kFairNone;
    }
    if (p >= V) return kFairBadWord;
    return p;
}

// index of the CSR entry (u, x), -1 if u has no such link
__device__ __forceinline__ int fair_edge_index(const int32_t *__restrict__ row_ptr,
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

// an extra constraint's index, -1 for none or for one outside [E, E + nextra)
__device__ __forceinline__ int fair_extra(const int32_t *__restrict__ extra, int64_t i, int j,
                                          int E, int nextra)
{
    if (!extra) return -1;
    const int x = extra[2 * i + j];
    return (x >= E && (int64_t)x < (int64_t)E + nextra) ? x : -1;
}

// a subtree sum: in global scratch the adds are L2 atomics, so the reads go there too
template <bool LDS>
__device__ __forceinline__ unsigned long long fair_sum(const unsigned long long *p)
{
    return LDS ? *p : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kFairLinkThreads) void fair_init_kernel(
    FairState s, const double *__restrict__ cap, int n_ent, int nlevel, int *__restrict__ err)
{
    const int i = (int)(blockIdx.x * (unsigned)kFairLinkThreads + threadIdx.x);
    if (i < n_ent) {
        double c = cap[i];
        if (!(c > 0.0) || __double_as_longlong(c) == (long long)kInfBits) {
            atomicOr(err, kErrFairRates);                  // not positive and finite
            c = __longlong_as_double((long long)kInfBits); // (never saturates: results invalid)
        }
        s.rem[i] = c;
        s.used[i] = 0.0;
        s.share[i] = __longlong_as_double((long long)kInfBits);
        s.n[i] = 0;
        s.n_prev[i] = 0;
    }
    if (i < nlevel) s.level[i] = kInfBits;
    if (i == 0) {
        *s.status = 0;
        *s.ticket = 0;
    }
}

// JT: u16 (LDS, none 0xFFFF) or u32 (global scratch, none 0xFFFFFFFF)
template <typename JT, bool LDS>
__global__ __launch_bounds__(kFairThreads) void fair_rows_kernel(
    FairRows t, int V, int E, int nextra, int nrows, int max_steps, int k,
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int64_t *__restrict__ pair_off, int64_t pair_lo, int64_t pair_hi,
    const int32_t *__restrict__ verts, const uint64_t *__restrict__ mult,
    const int32_t *__restrict__ extra, FairState s, double *__restrict__ rate,
    int32_t *__restrict__ bott, int32_t *__restrict__ round, unsigned char *__restrict__ scratch,
    size_t scratch_stride, int *__restrict__ err)
{
    extern __shared__ unsigned long long fair_lds[];
    __shared__ unsigned long long s_alive;
    constexpr JT kNone = (JT)~(JT)0;
    if (k > 0 && *s.status) return;                        // the rounds ended before this one
    const double r_prev =
        k > 0 ? __longlong_as_double((long long)s.level[k - 1]) : 0.0;
    const double inf = __longlong_as_double((long long)kInfBits);
    // generation g of the sums / ancestors: A0 + g * V, J0 + g * V; B aliases A
    unsigned long long *A0;
    if (LDS)
        A0 = fair_lds;
    else
        A0 = reinterpret_cast<unsigned long long *>(scratch + (size_t)blockIdx.x * scratch_stride);
    JT *J0 = reinterpret_cast<JT *>(A0 + 2 * (size_t)V);
    int *Ev = reinterpret_cast<int *>(J0 + 2 * (size_t)V);
    int *B0 = reinterpret_cast<int *>(A0);
    const int tid = (int)threadIdx.x;

    for (int r = (int)blockIdx.x; r < nrows; r += (int)gridDim.x) {
        const int64_t lo = pair_off[r], hi = pair_off[r + 1];
        if (lo < pair_lo || hi > pair_hi || hi < lo) {     // offsets outside the pair list
            if (tid == 0) atomicOr(err, kErrFairRates);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no flow)
        if (k > 0 && s.alive_row[r] == 0) continue;        // (uniform: none of them alive)
        const size_t rb = (size_t)r * (size_t)V;
        bool bad = false;

        // J_0 = parent, e_v = the link of v toward the root
        int any0 = 0;
        for (int v = tid; v < V; v += kFairThreads) {
            int slot;
            bool root;
            int p = fair_parent(t, rb, v, V, &slot, &root);
            int e = -1;
            if (p == kFairBadWord) {
                bad = true;
                p = kFairNone;
            }
            if (p >= 0) {
                if (t.to_root) {
                    e = fair_edge_index(row_ptr, col, v, p);
                } else if (t.layout == SDNR_TREE_SLOT) {
                    e = row_ptr[p] + slot;
                    if (e >= row_ptr[p + 1] || col[e] != v) e = -1;
                } else {
                    e = fair_edge_index(row_ptr, col, p, v);
                }
                if (e < 0 || e >= E) {                     // a tree link the graph does not have
                    bad = true;
                    e = -1;
                }
            }
            J0[v] = p < 0 ? kNone : (JT)p;
            Ev[v] = e;
            any0 |= p >= 0;
        }
        if (tid == 0) s_alive = 0;
        const int more0 = __syncthreads_or(any0);

        unsigned long long mine = 0;                       // this thread's flows still alive
        if (k == 0) {
            // classify the row's flows (rate 0.0, bott -1, round -1 are preset)
            for (int64_t i = lo + tid; i < hi; i += kFairThreads) {
                const int x = verts[i];
                if (x < 0 || x >= V) continue;
                if (mult && mult[i] == 0) continue;        // absent
                int slot;
                bool root;
                const int p = fair_parent(t, rb, x, V, &slot, &root);
                if (p < 0 && !root) continue;              // unreached in this row
                if (extra) {
                    const int x0 = extra[2 * i], x1 = extra[2 * i + 1];
                    if ((x0 != -1 && fair_extra(extra, i, 0, E, nextra) < 0) ||
                        (x1 != -1 && fair_extra(extra, i, 1, E, nextra) < 0))
                        atomicOr(err, kErrFairRates);      // (that constraint is ignored)
                }
                if (p < 0 && fair_extra(extra, i, 0, E, nextra) < 0 &&
                    fair_extra(extra, i, 1, E, nextra) < 0) {
                    rate[i] = inf;                         // no link and no extra
                    continue;
                }
                round[i] = kFairAlive;
                ++mine;
            }
        } else {
            // (a) the verdict of round k - 1: first saturated link toward the root
            for (int v = tid; v < V; v += kFairThreads) {
                const int e = Ev[v];
                B0[v] = (e >= 0 && s.share[e] == r_prev) ? e : -1;
            }
            __syncthreads();
            int cur = 0, steps = 0, more = more0;
            while (more && steps < max_steps) {
                const int *Bc = B0 + (cur ? V : 0);
                int *Bn = B0 + (cur ? 0 : V);
                const JT *Jc = J0 + (cur ? V : 0);
                JT *Jn = J0 + (cur ? 0 : V);
                int any = 0;
                for (int v = tid; v < V; v += kFairThreads) {
                    const JT j = Jc[v];
                    int b = Bc[v];
                    JT jj = kNone;
                    if (j != kNone) {
                        if (b < 0) b = Bc[j];
                        jj = Jc[j];
                        any |= jj != kNone;
                    }
                    Bn[v] = b;
                    Jn[v] = jj;
                }
                more = __syncthreads_or(any);
                cur ^= 1;
                ++steps;
            }
            const int *B = B0 + (cur ? V : 0);
            for (int64_t i = lo + tid; i < hi; i += kFairThreads) {
                if (round[i] != kFairAlive) continue;
                int b = B[verts[i]];
                if (b < 0) {
                    const int x0 = fair_extra(extra, i, 0, E, nextra);
                    const int x1 = fair_extra(extra, i, 1, E, nextra);
                    if (x0 >= 0 && s.share[x0] == r_prev) b = x0;
                    else if (x1 >= 0 && s.share[x1] == r_prev) b = x1;
                }
                if (b >= 0) {
                    rate[i] = r_prev;
                    bott[i] = b;
                    round[i] = k - 1;
                } else {
                    ++mine;
                }
            }
        }
        if (mine) atomicAdd(&s_alive, mine);
        __syncthreads();                                   // (B is read; A may be filled)
        const unsigned long long alive = s_alive;
        if (tid == 0) s.alive_row[r] = (long long)alive;
        // (bad is per thread; the row is dropped by all or none.  Only round 0
        // can find a bad row: later rounds skip it)
        int badrow = k == 0 ? __syncthreads_or(bad ? 1 : 0) : 0;
        int cur = 0;
        if (!badrow && alive) {
            // (b) A_0 = alive multiplicity, J_0 = parent again
            for (int v = tid; v < V; v += kFairThreads) {
                A0[v] = 0;
                if (k > 0) {
                    int slot;
                    bool root;
                    const int p = fair_parent(t, rb, v, V, &slot, &root);
                    J0[v] = p < 0 ? kNone : (JT)p;
                }
            }
            __syncthreads();
            for (int64_t i = lo + tid; i < hi; i += kFairThreads) {
                if (round[i] != kFairAlive) continue;
                const unsigned long long w = mult ? (unsigned long long)mult[i] : 1ull;
                atomicAdd(&A0[verts[i]], w);
            }
            __syncthreads();

            int steps = 0, more = more0;
            while (more) {
                if (steps == max_steps) {                      // an ancestor chain longer than V
                    bad = true;
                    break;
                }
                unsigned long long *Ac = A0 + (cur ? V : 0), *An = A0 + (cur ? 0 : V);
                JT *Jc = J0 + (cur ? V : 0), *Jn = J0 + (cur ? 0 : V);
                for (int v = tid; v < V; v += kFairThreads)
                    An[v] = fair_sum<LDS>(&Ac[v]);
                __syncthreads();
                int any = 0;
                for (int v = tid; v < V; v += kFairThreads) {
                    const JT j = Jc[v];
                    JT jj = kNone;
                    if (j != kNone) {
                        const unsigned long long a = fair_sum<LDS>(&Ac[v]);
                        if (a) atomicAdd(&An[j], a);
                        jj = Jc[j];
                        any |= jj != kNone;
                    }
                    Jn[v] = jj;
                }
                more = __syncthreads_or(any);
                cur ^= 1;
                ++steps;
            }
            badrow = __syncthreads_or(bad ? 1 : 0);
        }
        if (badrow) {
            // its flows stay 0.0 / -1 / -1
            for (int64_t i = lo + tid; i < hi; i += kFairThreads)
                if (round[i] == kFairAlive) round[i] = -1;
            if (tid == 0) {
                atomicOr(err, kErrFairRates);
                s.alive_row[r] = 0;
            }
            __syncthreads();                               // s_alive is reset by the next row
            continue;
        }
        if (alive == 0) {
            __syncthreads();
            continue;
        }

        // n[e_v] += T[v], n[extra] += mult
        const unsigned long long *T = A0 + (cur ? V : 0);
        for (int v = tid; v < V; v += kFairThreads) {
            const unsigned long long x = fair_sum<LDS>(&T[v]);
            const int e = Ev[v];
            if (x && e >= 0) atomicAdd(&s.n[e], x);
        }
        if (extra) {
            for (int64_t i = lo + tid; i < hi; i += kFairThreads) {
                if (round[i] != kFairAlive) continue;
                const unsigned long long w = mult ? (unsigned long long)mult[i] : 1ull;
                const int x0 = fair_extra(extra, i, 0, E, nextra);
                const int x1 = fair_extra(extra, i, 1, E, nextra);
                if (x0 >= 0) atomicAdd(&s.n[x0], w);
                if (x1 >= 0 && x1 != x0) atomicAdd(&s.n[x1], w);
            }
        }
        __syncthreads();                                   // the buffers are reused by the next row
    }
}

__global__ __launch_bounds__(kFairLinkThreads) void fair_links_kernel(FairState s, int n_ent, int k)
{
    // the multiply, the add and the subtract of step 2 round one by one, as the
    // host's numpy does: no fused multiply-add (HIP contracts by default, and
    // the __d*_rn intrinsics are plain operators that contract all the same)
#pragma clang fp contract(off)
    if (k > 0 && *s.status) return;                        // the rounds ended before this one
    const double inf = __longlong_as_double((long long)kInfBits);
    const int e = (int)(blockIdx.x * (unsigned)kFairLinkThreads + threadIdx.x);
    double sh = inf;
    if (e < n_ent) {
        const unsigned long long cnt = s.n[e];
        double rem = s.rem[e];
        if (k > 0) {
            const unsigned long long m = s.n_prev[e] - cnt;
            if (m) {
                const double r_prev = __longlong_as_double((long long)s.level[k - 1]);
                const double p = r_prev * (double)m;
                s.used[e] = s.used[e] + p;
                rem = fmax(rem - p, 0.0);
                s.rem[e] = rem;
            }
        }
        if (cnt) sh = rem / (double)cnt;
        s.share[e] = sh;
        s.n_prev[e] = cnt;
        s.n[e] = 0;
    }
    // rem >= 0 and cnt > 0: sh is a non-negative double or +inf, ordered as its bits
    unsigned long long bits = (unsigned long long)__double_as_longlong(sh);
    for (int d = SDNR_WAVE / 2; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(bits, d, SDNR_WAVE);
        bits = o < bits ? o : bits;
    }
    if (lane_id() == 0 && bits != kInfBits) atomicMin(&s.level[k], bits);
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(s.ticket, 1u) == gridDim.x - 1) {    // the last workgroup of the pass
            __threadfence();
            *s.ticket = 0;
            if (__hip_atomic_load(&s.level[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                kInfBits)
                *s.status = (unsigned long long)k + 1;
        }
    }
}

}  // namespace

int sdnr_launch_fair_rates(sdnr_ctx *ctx, const void *d_tree, int32_t layout, bool to_root,
                           int32_t nrows, const int64_t *d_pair_off, int64_t pair_lo,
                           int64_t pair_hi, const int32_t *d_verts, const uint64_t *d_mult,
                           const int32_t *d_extra, const double *d_cap, int32_t nextra,
                           double *d_rate, int32_t *d_bott, int32_t *d_round, double *d_level,
                           int32_t max_rounds, double *d_used, int32_t *nrounds)
{
    const int V = ctx->V;
    const int n_ent = ctx->E + nextra;
    const size_t npairs = (size_t)(pair_hi - pair_lo);
    int max_steps = 1;                                     // ceil(log2 V) + 1
    while ((1ll << (max_steps - 1)) < (long long)V) ++max_steps;

    // the row kernel's shape, and its per-workgroup scratch slices
    const bool lds_form = V <= kFairLdsMaxV;
    const size_t lds = lds_form ? (size_t)V * kFairBytesPerV : 0;
    const size_t stride = lds_form ? 0 : ((((size_t)V * 28) + 255) & ~(size_t)255);
    int64_t g;
    if (lds_form) {
        int per_cu = (int)(SDNR_LDS_PER_CU / (lds ? lds : 1));
        per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);     // 2048 threads per CU
        g = (int64_t)ctx->num_cus * per_cu;
    } else {
        g = ctx->num_cus;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
    }
    if (g > nrows) g = nrows;

    // the state behind the slices: n, n_prev, rem, share, level, alive_row, status, ticket
    const size_t slices = (stride * (size_t)g + 255) & ~(size_t)255;
    const size_t nlevel = (size_t)max_rounds + 1;
    const size_t state = 8 * (4 * (size_t)n_ent + nlevel + (size_t)nrows + 2);
    const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, slices + state);
    if (rc) return rc;
    unsigned char *base = static_cast<unsigned char *>(ctx->scratch);
    unsigned long long *w = reinterpret_cast<unsigned long long *>(base + slices);
    FairState s;
    s.n = w;
    s.n_prev = s.n + n_ent;
    s.rem = reinterpret_cast<double *>(s.n_prev + n_ent);
    s.share = s.rem + n_ent;
    s.level = reinterpret_cast<unsigned long long *>(s.share + n_ent);
    s.alive_row = reinterpret_cast<long long *>(s.level + nlevel);
    s.status = reinterpret_cast<unsigned long long *>(s.alive_row + nrows);
    s.ticket = reinterpret_cast<unsigned int *>(s.status + 1);
    s.used = d_used;

    FairRows t{static_cast<const uint32_t *>(d_tree), layout, to_root ? 1 : 0};
    hipStream_t st = ctx->stream;
    // every flow reads 0.0 / -1 / -1 until a row says otherwise
    SDNR_HIP(hipMemsetAsync(d_rate + pair_lo, 0, npairs * sizeof(double), st));
    SDNR_HIP(hipMemsetAsync(d_bott + pair_lo, 0xFF, npairs * sizeof(int32_t), st));
    SDNR_HIP(hipMemsetAsync(d_round + pair_lo, 0xFF, npairs * sizeof(int32_t), st));
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, st));
    const size_t init_n = (size_t)n_ent > nlevel ? (size_t)n_ent : nlevel;
    unsigned link_blocks = (unsigned)((n_ent + kFairLinkThreads - 1) / kFairLinkThreads);
    if (link_blocks == 0) link_blocks = 1;                 // (no link, no extra: level[0] = +inf)
    hipLaunchKernelGGL(fair_init_kernel,
                       dim3((unsigned)((init_n + kFairLinkThreads - 1) / kFairLinkThreads)),
                       dim3(kFairLinkThreads), 0, st, s, d_cap, n_ent, (int)nlevel, ctx->d_err);
    SDNR_HIP(hipGetLastError());
    int launches = 1;
    auto fn_lds = fair_rows_kernel<uint16_t, true>;
    if (lds_form) sdnr_allow_lds(reinterpret_cast<const void *>(fn_lds), lds);
    ctx->last_kernel = lds_form ? "fair_rows_kernel<lds>" : "fair_rows_kernel<global>";
    ctx->last_grid = g;

    int k = 0, done = -1;
    while (done < 0) {
        // rounds 0 .. max_rounds: the last one only applies the verdict of
        // round max_rounds - 1 and makes used final
        const int end = k + kFairBatch <= max_rounds + 1 ? k + kFairBatch : max_rounds + 1;
        for (; k < end; ++k) {
            if (lds_form)
                hipLaunchKernelGGL(fn_lds, dim3((unsigned)g), dim3(kFairThreads), lds, st, t, V,
                                   ctx->E, nextra, nrows, max_steps, k, ctx->row_ptr, ctx->col,
                                   d_pair_off, pair_lo, pair_hi, d_verts, d_mult, d_extra, s,
                                   d_rate, d_bott, d_round, (unsigned char *)nullptr, (size_t)0,
                                   ctx->d_err);
            else
                hipLaunchKernelGGL((fair_rows_kernel<uint32_t, false>), dim3((unsigned)g),
                                   dim3(kFairThreads), 0, st, t, V, ctx->E, nextra, nrows,
                                   max_steps, k, ctx->row_ptr, ctx->col, d_pair_off, pair_lo,
                                   pair_hi, d_verts, d_mult, d_extra, s, d_rate, d_bott, d_round,
                                   base, stride, ctx->d_err);
            hipLaunchKernelGGL(fair_links_kernel, dim3(link_blocks), dim3(kFairLinkThreads), 0, st,
                               s, n_ent, k);
            launches += 2;
        }
        SDNR_HIP(hipGetLastError());
        int word[2];
        const int rf = sdnr_fetch_ints(ctx, reinterpret_cast<const int *>(s.status), 2, word);
        if (rf) return rf;
        const unsigned long long status =
            ((unsigned long long)(uint32_t)word[1] << 32) | (uint32_t)word[0];
        if (status) done = (int)(status - 1);
        else if (k > max_rounds) done = max_rounds;        // flows left alive keep round -2
    }
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, st));
    if (max_rounds > 0)
        SDNR_HIP(hipMemcpyAsync(d_level, s.level, (size_t)max_rounds * sizeof(double),
                                hipMemcpyDeviceToDevice, st));
    ctx->last_launches = launches;
    *nrounds = done < max_rounds ? done : max_rounds;
    return SDNR_OK;
}
