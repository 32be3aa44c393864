// lfa_tables.hip -- loop-free alternate (fast-reroute) backup next hops.
//
// For a destination d and a switch s with primary next hop p (the first tight
// link of s's ascending row, sdnr_cost_tables' nh), a neighbour n != p of
// finite P[d][n] may take d's traffic the moment the link s -> p dies iff no
// least-cost route n -> d comes back through s (RFC 5286 inequality 1):
//   loop-free        P[s][n] == INF  or  P[d][n] < P[s][n] + P[d][s]
//   downstream       P[d][n] < P[d][s]
//   node-protecting  loop-free and (P[p][n] == INF or P[d][n] < P[p][n] + P[d][p])
// with P[d][x] the least cost x -> d, row d of the caller's all-pairs table
// (sdnr_cost_tables over dst = 0..V-1).  The backup is the loop-free candidate
// of the smallest key (not node-protecting, cost[e] + P[d][n], n) -- without
// the first component under SDNR_LFA_LINK_ONLY.  Everything is integer: two
// table entries may sum to 2^32 or more, so the sums are u64, and INF enters
// none of them.
//
// Scope: V <= kLfaMaxV = 16,384 (sdnr_apsp's cap: the table is 1 GiB there and
// one u32 row 64 KiB of LDS).  The fat-tree k=48 (2,880 switches) and the
// dragonfly a16 h8 p8 (2,064) fit; the torus 32^3 and the 100k Jellyfish cannot
// hold an all-pairs table and are out of scope.
//
// Two of the three table reads look like gathers across rows of P but do not
// depend on the destination: back[e] = P[s][n] belongs to the link, and
// P[p][n] to a pair of neighbours of s.  A pre-pass gathers both once per call
// into the context scratch -- back[E] and, per vertex, the deg x deg matrix
// nn[off[s] + j * deg + i] = P[col[lo + j]][col[lo + i]], i fastest, so the
// candidates of one primary (slot j) are one contiguous line.  The main kernel
// then reads LDS (the destination's row) and contiguous streams only: col,
// cost, back and one nn line per vertex.
//
// Main kernel: one workgroup per destination row, persistent over the rows,
// the row P[d][.] staged in LDS.  A wavefront takes 64 consecutive vertices;
// each of its eight 8-lane groups takes one vertex at a time and strides the
// vertex's out-row 8 links at a time (any degree: a 130-link hub is 17
// strides), first for the primary's slot (ballot, first tight link), then for
// the smallest key (u64 min over the group).  Group g handles vertex
// 64 * blk + 8 * g + it in turn it, and lane 8 * g + it keeps that result:
// after 8 turns lane l holds vertex 64 * blk + l and the three tables are
// stored 64 entries wide.  A turn is a chain of dependent loads -- latency, not
// bandwidth --, so what does not depend on the scan leaves the chain: the row
// bounds, P[d][s] and the matrix offset of the 64 vertices are read once per
// block, lane l for vertex l, and fetched per turn by a lane shuffle; the
// primary and its cost come from the lane that found it; the winner's vertex
// and port are read once per block, by the lane that stores them.  The group
// width trades vertices in flight against strides per row: 8 lanes ran the
// k=48 fat-tree's 2,880 rows in 1.05 ms, 16 in 1.26, 4 in 1.30, 32 in 2.0 and
// 2 in 2.35.
#include "common.h"

namespace {

constexpr int kLfaThreads = 1024;
#ifdef SDNR_LFA_GROUP                              // A/B builds of the widths measured
constexpr int kLfaGroup = SDNR_LFA_GROUP;
#else
constexpr int kLfaGroup = 8;                       // lanes per vertex
#endif
static_assert(kLfaGroup >= 2 && kLfaGroup <= 32 && SDNR_WAVE % kLfaGroup == 0,
              "a group's ballot is a u32");
constexpr uint32_t kLfaGroupMask = (uint32_t)(~(uint64_t)0 >> (64 - kLfaGroup));
constexpr int kLfaGroups = SDNR_WAVE / kLfaGroup;  // vertices in flight per wavefront
constexpr uint32_t kLfaInf = SDNR_COST_INF;
constexpr int kPreThreads = 256;

// off[v] = sum of deg(u)^2 over u < v (one workgroup; V <= 16 * 1024)
__global__ __launch_bounds__(kLfaThreads) void lfa_offsets_kernel(
    int V, const int32_t *__restrict__ row_ptr, uint32_t *__restrict__ off)
{
    __shared__ uint32_t part[kLfaThreads];
    const int tid = (int)threadIdx.x;
    const int per = (V + kLfaThreads - 1) / kLfaThreads;
    const int lo = tid * per < V ? tid * per : V;
    const int hi = lo + per < V ? lo + per : V;
    uint32_t sum = 0;
    for (int v = lo; v < hi; ++v) {
        const uint32_t g = (uint32_t)(row_ptr[v + 1] - row_ptr[v]);
        sum += g * g;
    }
    part[tid] = sum;
    __syncthreads();
    for (int st = 1; st < kLfaThreads; st <<= 1) {
        const uint32_t t = tid >= st ? part[tid - st] : 0u;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
    for (int v = lo; v < hi; ++v) {
        off[v] = run;
        const uint32_t g = (uint32_t)(row_ptr[v + 1] - row_ptr[v]);
        run += g * g;
    }
}

// back[e] = P[s][n]; nn[off[s] + j * deg + i] = P[n_j][n_i].  One wavefront
// per vertex, each of its groups on one line of the matrix at a time.
template <bool NN>
__global__ __launch_bounds__(kPreThreads) void lfa_prepass_kernel(
    int V, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const uint32_t *__restrict__ pall, const uint32_t *__restrict__ off,
    uint32_t *__restrict__ back, uint32_t *__restrict__ nn)
{
    const int s = (int)blockIdx.x * (kPreThreads / SDNR_WAVE) + ((int)threadIdx.x >> 6);
    if (s >= V) return;
    const int lane = (int)threadIdx.x & 63;
    const int lo = row_ptr[s], deg = row_ptr[s + 1] - lo;
    const uint32_t *ps = pall + (size_t)s * (size_t)V;
    for (int i = lane; i < deg; i += SDNR_WAVE) back[lo + i] = ps[col[lo + i]];
    if (NN) {
        const int g = lane / kLfaGroup, sub = lane % kLfaGroup;
        uint32_t *mat = nn + off[s];
        for (int j = g; j < deg; j += kLfaGroups) {
            const uint32_t *pj = pall + (size_t)col[lo + j] * (size_t)V;
            for (int i = sub; i < deg; i += kLfaGroup) mat[(size_t)j * deg + i] = pj[col[lo + i]];
        }
    }
}

// NP: node protection evaluated (nn lines read); GATHER: P[s][n] and P[p][n]
// straight from pall instead of the pre-pass arrays (the measured alternative,
// DESIGN.md 4.13)
template <bool NP, bool GATHER>
__global__ __launch_bounds__(kLfaThreads) void lfa_tables_kernel(
    int V, int ndst, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ port, const uint32_t *__restrict__ cost,
    const uint32_t *__restrict__ pall, const uint32_t *__restrict__ back,
    const uint32_t *__restrict__ nn, const uint32_t *__restrict__ off,
    const int32_t *__restrict__ dst, int32_t *__restrict__ backup,
    int32_t *__restrict__ backup_port, uint8_t *__restrict__ kind, uint32_t *__restrict__ counts,
    int *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lfa_row[];
    __shared__ uint32_t cnt[4];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int g = lane / kLfaGroup, sub = lane % kLfaGroup;
    const int nblk = (V + SDNR_WAVE - 1) / SDNR_WAVE;

    for (int r = (int)blockIdx.x; r < ndst; r += (int)gridDim.x) {
        const int dr = dst[r];
        const bool ok = dr >= 0 && dr < V;                 // else: an empty row
        const int d = ok ? dr : 0;
        const uint32_t *pd = pall + (size_t)d * (size_t)V;
        for (int x = tid; x < V; x += kLfaThreads) lfa_row[x] = ok ? pd[x] : kLfaInf;
        if (tid < 4) cnt[tid] = 0;
        __syncthreads();
        if (ok && tid == 0 && lfa_row[d] != 0) atomicOr(err, kErrLfa);

        uint32_t c_prim = 0, c_back = 0, c_np = 0, c_down = 0;      // wave-uniform
        for (int blk = wave; blk < nblk; blk += kLfaThreads / SDNR_WAVE) {
            // lane l reads vertex 64 * blk + l's row bounds, cost and matrix
            // offset once; a turn fetches its vertex's from the lane that holds it
            const int v = blk * SDNR_WAVE + lane;
            int l_lo = 0, l_deg = 0;
            uint32_t l_P = kLfaInf, l_off = 0;
            if (v < V) {
                l_lo = row_ptr[v];
                l_deg = row_ptr[v + 1] - l_lo;
                l_P = lfa_row[v];
                if (NP && !GATHER) l_off = off[v];
            }
            int my_e = -1;                                  // the backup's link
            uint32_t my_kind = 0;
            bool my_prim = false;
            for (int it = 0; it < kLfaGroup; ++it) {
                // group-uniform from here: one vertex per group of kLfaGroup lanes
                const int from = g * kLfaGroup + it;
                const int s = blk * SDNR_WAVE + from;
                const int lo = __shfl(l_lo, from), deg = __shfl(l_deg, from);
                const uint32_t Ps = (uint32_t)__shfl((int)l_P, from);
                const uint32_t offs = (uint32_t)__shfl((int)l_off, from);
                int win = -1;
                uint32_t k = 0;
                bool prim = false;
                if (ok && s != d && Ps != kLfaInf) {
                    // 1. the primary's slot: the first tight link of the row
                    int jp = -1, p = 0;
                    uint32_t Pp = 0;
                    for (int base = 0; base < deg; base += kLfaGroup) {
                        const int i = base + sub;
                        int n = 0;
                        uint32_t Pn = kLfaInf;
                        bool tight = false;
                        if (i < deg) {
                            n = col[lo + i];
                            Pn = lfa_row[n];
                            const uint32_t c = cost ? cost[lo + i] : 1u;
                            tight = Pn != kLfaInf && (uint64_t)Pn + c == (uint64_t)Ps;
                        }
                        const uint32_t m = (uint32_t)(__ballot(tight) >> (g * kLfaGroup)) &
                                           kLfaGroupMask;
                        if (m) {
                            const int at = __builtin_ctz(m);
                            jp = base + at;
                            p = __shfl(n, g * kLfaGroup + at);
                            Pp = (uint32_t)__shfl((int)Pn, g * kLfaGroup + at);
                            break;
                        }
                    }
                    if (jp < 0) {
                        // finite cost > 0 and no tight link: no labelling of this graph
                        if (Ps != 0 && sub == 0) atomicOr(err, kErrLfa);
                    } else {
                        prim = true;
                        // 2. the loop-free candidate of the smallest key
                        //    not-np << 51 | (cost + Pn) << 17 | slot << 1 | downstream
                        const uint32_t *line = nullptr;
                        if (NP) line = GATHER ? pall + (size_t)p * (size_t)V
                                              : nn + offs + (size_t)jp * deg;
                        const uint32_t *ps = GATHER ? pall + (size_t)s * (size_t)V : back + lo;
                        uint64_t best = ~(uint64_t)0;
                        for (int base = 0; base < deg; base += kLfaGroup) {
                            const int i = base + sub;
                            if (i >= deg || i == jp) continue;
                            const int n = col[lo + i];
                            const uint32_t Pn = lfa_row[n];
                            if (Pn == kLfaInf) continue;
                            const uint32_t bk = ps[GATHER ? n : i];
                            if (bk != kLfaInf && (uint64_t)Pn >= (uint64_t)bk + Ps) continue;
                            uint64_t notnp = 0;
                            if (NP) {
                                const uint32_t q = line[GATHER ? n : i];
                                notnp = (q != kLfaInf && (uint64_t)Pn >= (uint64_t)q + Pp) ? 1 : 0;
                            }
                            const uint32_t c = cost ? cost[lo + i] : 1u;
                            const uint64_t key = notnp << 51 | ((uint64_t)Pn + c) << 17 |
                                                 (uint64_t)i << 1 | (Pn < Ps ? 1u : 0u);
                            best = key < best ? key : best;
                        }
#pragma unroll
                        for (int w = kLfaGroup / 2; w > 0; w >>= 1) {
                            const uint64_t o = __shfl_xor((unsigned long long)best, w, kLfaGroup);
                            best = o < best ? o : best;
                        }
                        if (best != ~(uint64_t)0) {
                            win = lo + ((int)(best >> 1) & 0xFFFF);
                            k = 1u | ((uint32_t)best & 1u) << 1 |
                                ((NP && !(best >> 51)) ? 4u : 0u);
                        }
                    }
                }
                if (sub == it) {
                    my_e = win;
                    my_kind = k;
                    my_prim = prim;
                }
            }
            // lane l holds vertex 64 * blk + l
            if (v < V) {
                const size_t o = (size_t)r * (size_t)V + (size_t)v;
                backup[o] = my_e < 0 ? -1 : col[my_e];
                backup_port[o] = my_e < 0 ? -1 : port[my_e];
                kind[o] = (uint8_t)my_kind;
            }
            c_prim += (uint32_t)__popcll(__ballot(my_prim));
            c_back += (uint32_t)__popcll(__ballot((my_kind & 1u) != 0));
            c_np += (uint32_t)__popcll(__ballot((my_kind & 4u) != 0));
            c_down += (uint32_t)__popcll(__ballot((my_kind & 2u) != 0));
        }
        if (counts) {
            if (lane == 0) {
                atomicAdd(&cnt[0], c_prim);
                atomicAdd(&cnt[1], c_back);
                atomicAdd(&cnt[2], c_np);
                atomicAdd(&cnt[3], c_down);
            }
            __syncthreads();
            if (tid < 4) counts[(size_t)r * 4 + tid] = cnt[tid];
        }
        __syncthreads();                                   // the row is reused by the next one
    }
}

template <bool NP, bool GATHER>
int launch_main(sdnr_ctx *ctx, const char *name, const uint32_t *cost, const uint32_t *d_pall,
                const uint32_t *back, const uint32_t *nn, const uint32_t *off,
                const int32_t *d_dst, int32_t ndst, int32_t *d_backup, int32_t *d_backup_port,
                uint8_t *d_kind, uint32_t *d_counts)
{
    const int V = ctx->V;
    const size_t lds = (((size_t)V * sizeof(uint32_t)) + 15) & ~(size_t)15;
    auto fn = lfa_tables_kernel<NP, GATHER>;
    sdnr_allow_lds(reinterpret_cast<const void *>(fn), lds);
    int64_t g = (int64_t)ctx->num_cus * 2;                 // 2048 threads per CU
    if (g > ndst) g = ndst;
    ctx->last_kernel = name;
    ctx->last_launches = 1;
    ctx->last_grid = g;
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kLfaThreads), lds, ctx->stream, V, ndst,
                       ctx->row_ptr, ctx->col, ctx->port, cost, d_pall, back, nn, off, d_dst,
                       d_backup, d_backup_port, d_kind, d_counts, ctx->d_err);
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}

}  // namespace

int sdnr_launch_lfa_tables(sdnr_ctx *ctx, const uint32_t *d_pall, const int32_t *d_dst,
                           int32_t ndst, int32_t *d_backup, int32_t *d_backup_port,
                           uint8_t *d_kind, uint32_t *d_counts, bool link_only)
{
    const int V = ctx->V;
    const size_t E = (size_t)ctx->E;
    const uint32_t *cost = ctx->has_cost ? ctx->cost : nullptr;    // none: every link costs 1
#ifdef SDNR_DIAG_VARIANTS
    // the measured alternative (diagnostic build only, SDNROUTE_LFA_GATHER=1):
    // no pre-pass, P[s][n] and P[p][n] gathered from pcost_all by the main
    // kernel -- slower on both bench fabrics
    const char *f = sdnr_tune_env("SDNROUTE_LFA_GATHER");
    if (f && f[0] == '1') {
        if (link_only)
            return launch_main<false, true>(ctx, "lfa_tables_kernel<link,gather>", cost, d_pall,
                                            nullptr, nullptr, nullptr, d_dst, ndst, d_backup,
                                            d_backup_port, d_kind, d_counts);
        return launch_main<true, true>(ctx, "lfa_tables_kernel<node,gather>", cost, d_pall, nullptr,
                                       nullptr, nullptr, d_dst, ndst, d_backup, d_backup_port,
                                       d_kind, d_counts);
    }
#endif
    // scratch: back[E] | off[V] | nn[sum of deg^2], each 256-byte aligned
    const size_t nn_bytes = link_only ? 0 : (size_t)ctx->deg2_sum * sizeof(uint32_t);
    if (nn_bytes > kLoadsScratchBytes)
        return sdnr_fail(SDNR_ERR_NOMEM, "sdnr_lfa_tables: the neighbour-pair matrices take "
                         "%zu bytes (4 per squared out-degree), above the %zu of scratch: pass "
                         "SDNR_LFA_LINK_ONLY for link-protecting alternates", nn_bytes,
                         kLoadsScratchBytes);
    const size_t back_bytes = (E * sizeof(uint32_t) + 255) & ~(size_t)255;
    const size_t off_bytes = ((size_t)V * sizeof(uint32_t) + 255) & ~(size_t)255;
    const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes,
                                back_bytes + off_bytes + nn_bytes);
    if (rc) return rc;
    char *base = static_cast<char *>(ctx->scratch);
    uint32_t *back = reinterpret_cast<uint32_t *>(base);
    uint32_t *off = reinterpret_cast<uint32_t *>(base + back_bytes);
    uint32_t *nn = reinterpret_cast<uint32_t *>(base + back_bytes + off_bytes);
    const unsigned pre_grid = (unsigned)((V + kPreThreads / SDNR_WAVE - 1) /
                                         (kPreThreads / SDNR_WAVE));
    if (link_only) {
        hipLaunchKernelGGL(lfa_prepass_kernel<false>, dim3(pre_grid), dim3(kPreThreads), 0,
                           ctx->stream, V, ctx->row_ptr, ctx->col, d_pall, off, back, nn);
        SDNR_HIP(hipGetLastError());
        return launch_main<false, false>(ctx, "lfa_tables_kernel<link>", cost, d_pall, back, nn,
                                         off, d_dst, ndst, d_backup, d_backup_port, d_kind,
                                         d_counts);
    }
    hipLaunchKernelGGL(lfa_offsets_kernel, dim3(1), dim3(kLfaThreads), 0, ctx->stream, V,
                       ctx->row_ptr, off);
    hipLaunchKernelGGL(lfa_prepass_kernel<true>, dim3(pre_grid), dim3(kPreThreads), 0, ctx->stream,
                       V, ctx->row_ptr, ctx->col, d_pall, off, back, nn);
    SDNR_HIP(hipGetLastError());
    return launch_main<true, false>(ctx, "lfa_tables_kernel<node>", cost, d_pall, back, nn, off,
                                    d_dst, ndst, d_backup, d_backup_port, d_kind, d_counts);
}
