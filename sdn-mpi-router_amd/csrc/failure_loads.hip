// failure_loads.hip -- link-failure what-if loads: the ECMP-over-least-cost
// link loads of a traffic matrix once per failure scenario, the uploaded graph
// and costs untouched.
//
// A scenario is a list of failed directed links (CSR edge indices, ascending).
// A work item is (scenario k, destination row r): one workgroup, persistent
// over the items, runs all of cost_tables.hip + cost_ecmp_loads.hip for that
// destination on the graph WITHOUT the scenario's links, the row state in LDS
// from start to end -- no table goes to HBM:
//   1. mask   flag[x] = 1 for every vertex x with a failed out-link (the
//             source of failed edge f is found by bisection in row_ptr);
//   2. pcost  pull Bellman-Ford from pcost[d] = 0 over the links not masked,
//             as cost_tables.hip argues it: one writer per word, values that
//             only decrease, a sweep that changes nothing read the fixed
//             point; at most V sweeps (costs >= 1).  A vertex whose value is
//             <= the number of sweeps done is final (its least-cost route has
//             no more links than that) and skips its walk, so a vertex walks
//             its row about once per level, not once per sweep.  Without
//             uploaded costs every link costs 1: hop counts;
//   3. order  depth[x] = the longest next-hop chain from x and the route
//             counts sigma[], by the pull sweeps of cost_ecmp_loads.hip;
//   4. push   the row's demand enters at its sources and is pushed down by
//             descending depth; loads go to load[k * E + e] with f64 atomics;
//   5. reach  routed[k][i] = the pair's source has a finite masked pcost;
//             lost[k] += the weights of the pairs that have none.
// The mask is applied in EVERY row walk, not only in the Bellman-Ford: a
// failed link x -> n can stay arithmetically tight (pcost[n] + cost == pcost[x]
// still holds when x has another next hop of the same cost), so a push that
// tested costs alone would send traffic over the dead link.
//
// Mask form.  The failed list stays where the caller put it (global memory; a
// scenario is a few words, L2 / K$ resident) and only the per-vertex flag byte
// is row state.  A vertex without the flag -- nearly all of them -- pays one
// integer compare per edge (e against a "next failed edge" register that holds
// INT_MAX).  A flagged vertex bisects the sorted list once per walk for its
// first edge index (its edges are contiguous in edge order) and merges along
// the walk; duplicates are skipped by the same merge.  Indices outside [0, E)
// match no edge, hence are ignored by construction (and reported).
//
// No NaN or Inf is ever formed, by the rules of cost_ecmp_loads.hip.  A failed
// index outside [0, E), a list that is not ascending, offsets outside their
// lists, sweeps that outrun V and a sigma above the double range raise the
// context's error word.
//
// Row state: LDS (f64 sigma + f64 flow + u32 pcost + u16 depth + u8 flag, 23
// bytes per vertex) up to kFailureLdsMaxV vertices, else a per-workgroup slice
// of the context scratch (the depths u32: 25 bytes per vertex), all of it read
// and written with agent-scope relaxed accesses.
#include "common.h"
#include "rowstate.h"

namespace {

// as cost_tables.hip and cost_ecmp_loads.hip: chains of dependent LDS / L2
// reads per thread, the waves that hide them come from the workgroup
constexpr int kFailThreads = 1024;
constexpr uint32_t kFailInf = SDNR_COST_INF;
constexpr int kNoFail = 0x7FFFFFFF;

// The failed links of one scenario, fail[0 .. hi) ascending, seen from the row
// walk of one vertex.  dead(e): is edge e failed -- e ascends along the walk,
// the cursor follows.
struct FailCursor {
    const int32_t *fail;
    int hi, at, next;

    // flagged: the walk of a vertex with failed out-links starts at its first
    // edge e0 -- the first entry >= e0 by bisection; else nothing ever matches
    __device__ __forceinline__ FailCursor(bool flagged, const int32_t *f, int n, int e0)
        : fail(f), hi(n), at(n), next(kNoFail)
    {
        if (!flagged) return;
        int a = 0, b = n;
        while (a < b) {
            const int m = a + ((b - a) >> 1);
            if (f[m] < e0) a = m + 1;
            else b = m;
        }
        at = a;
        if (a < n) next = f[a];
    }
    __device__ __forceinline__ bool dead(int e)
    {
        if (e < next) return false;                        // (always, without the flag)
        bool hit = false;
        do {                                               // duplicates; at <= hi: it ends
            hit |= next == e;
            ++at;
            next = at < hi ? fail[at] : kNoFail;
        } while (next <= e);
        return hit;
    }
};

// hop: sigma[x] holds the number of next hops instead of the route count
template <bool LDS>
__global__ __launch_bounds__(kFailThreads) void failure_ecmp_loads_kernel(
    int V, int E, int nrows, int nscen, int hop, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const uint32_t *__restrict__ cost,
    const int32_t *__restrict__ dst, const int64_t *__restrict__ pair_off, int64_t pair_lo,
    int64_t pair_hi, const int32_t *__restrict__ srcs, const uint64_t *__restrict__ weight,
    const int64_t *__restrict__ scen_off, int64_t scen_lo, int64_t scen_hi,
    const int32_t *__restrict__ scen_edges, double *__restrict__ load, double *__restrict__ lost,
    unsigned char *__restrict__ routed, unsigned char *__restrict__ scratch,
    size_t scratch_stride, int *__restrict__ err)
{
    typedef FailDepth<LDS> Dp;
    typedef typename Dp::T depth_t;
    // sigma f64 [V] | flow f64 [V] | pcost u32 [V] | depth u16 / u32 [V] | flag u8 [V]
    extern __shared__ __attribute__((aligned(16))) unsigned char failure_lds[];
    unsigned char *base = LDS ? failure_lds : scratch + (size_t)blockIdx.x * scratch_stride;
    double *sigma = reinterpret_cast<double *>(base);
    double *flow = sigma + V;
    uint32_t *pc = reinterpret_cast<uint32_t *>(flow + V);
    depth_t *depth = reinterpret_cast<depth_t *>(pc + V);
    uint8_t *flag = reinterpret_cast<uint8_t *>(depth + V);
    const int tid = (int)threadIdx.x;
    const int64_t npairs = pair_hi - pair_lo;
    const int64_t nitems = (int64_t)nscen * (int64_t)nrows;

    for (int64_t item = (int64_t)blockIdx.x; item < nitems; item += (int64_t)gridDim.x) {
        const int k = (int)(item / nrows), r = (int)(item % nrows);
        const int64_t lo = pair_off[r], hi = pair_off[r + 1];
        if (lo < pair_lo || hi > pair_hi || hi < lo) {     // offsets outside the pair list
            if (tid == 0) atomicOr(err, kErrFailureLoads);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no demand)
        const int64_t flo64 = scen_off[k], fhi64 = scen_off[k + 1];
        if (flo64 < scen_lo || fhi64 > scen_hi || fhi64 < flo64 ||
            fhi64 - flo64 > (int64_t)0x7FFFFFF0) {         // ... outside the scenario list
            if (tid == 0) atomicOr(err, kErrFailureLoads);
            continue;
        }
        const int32_t *fail = scen_edges + flo64;          // (never read when nfail == 0)
        const int nfail = (int)(fhi64 - flo64);
        int d = dst[r];
        if (d < 0 || d >= V) d = -1;                       // no vertex: an empty row
        // routed[k][i - pair_lo]
        unsigned char *rt = routed ? routed + (size_t)k * (size_t)npairs : nullptr;

        if (d < 0) {                                       // (uniform) nothing routed, all lost
            double gone = 0.0;
            for (int64_t i = lo + tid; i < hi; i += kFailThreads) {
                if (rt) rt[i - pair_lo] = 0;
                const int s = srcs[i];
                if (s < 0 || s >= V) continue;
                const uint64_t w = weight ? weight[i] : 1ull;
                if (w) gone += (double)w;
            }
            if (lost && gone > 0.0) atomicAdd(&lost[k], gone);
            continue;
        }

        // 1. pcost[d] = 0, INF elsewhere; no flags
        for (int x = tid; x < V; x += kFailThreads) {
            fl_st<LDS, uint32_t>(&pc[x], x == d ? 0u : kFailInf);
            fl_st<LDS, uint8_t>(&flag[x], (uint8_t)0);
        }
        __syncthreads();
        //    ... flag the source vertex of every failed link
        for (int i = tid; i < nfail; i += kFailThreads) {
            const int f = fail[i];
            if (i > 0 && fail[i - 1] > f) atomicOr(err, kErrFailureLoads);   // not ascending
            if (f < 0 || f >= E) {                         // no link: ignored, reported
                atomicOr(err, kErrFailureLoads);
                continue;
            }
            int a = 0, b = V;                              // the x with row_ptr[x] <= f < row_ptr[x + 1]
            while (b - a > 1) {
                const int m = a + ((b - a) >> 1);
                if (row_ptr[m] <= f) a = m;
                else b = m;
            }
            fl_st<LDS, uint8_t>(&flag[a], (uint8_t)1);
        }
        __syncthreads();

        // 2. least costs: sweeps until one changes nothing
        bool done = false;
        for (int sweep = 0; sweep < V; ++sweep) {
            int changed = 0;
            for (int x = tid; x < V; x += kFailThreads) {
                const uint32_t cur = fl_ld<LDS, uint32_t>(&pc[x]);
                // costs are >= 1: a route of cost <= sweep has <= sweep links, and after
                // `sweep` sweeps every vertex with such a least-cost route is final
                if (cur <= (uint32_t)sweep) continue;
                uint32_t best = cur;
                const int e0 = row_ptr[x], re = row_ptr[x + 1];
                if (!fl_ld<LDS, uint8_t>(&flag[x])) {       // nearly every vertex: the bare walk
#pragma unroll 4
                    for (int e = e0; e < re; ++e) {
                        const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[col[e]]);
                        const uint32_t t = pn + (cost ? cost[e] : 1u);   // (unused when pn is INF)
                        if (pn != kFailInf && t < best) best = t;
                    }
                } else {
                    FailCursor fc(true, fail, nfail, e0);
                    for (int e = e0; e < re; ++e) {
                        if (fc.dead(e)) continue;
                        const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[col[e]]);
                        const uint32_t t = pn + (cost ? cost[e] : 1u);
                        if (pn != kFailInf && t < best) best = t;
                    }
                }
                if (best != cur) {
                    fl_st<LDS, uint32_t>(&pc[x], best);
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) {
                done = true;
                break;
            }
        }
        if (!done) {                                       // (uniform) costs the upload refuses
            if (tid == 0) atomicOr(err, kErrFailureLoads);
            continue;
        }

        // 3a. flow = 0; the destination and the unreachable are final at depth 0
        for (int x = tid; x < V; x += kFailThreads) {
            const uint32_t px = fl_ld<LDS, uint32_t>(&pc[x]);
            fl_st_f64<LDS>(&sigma[x], (px == 0 && !hop) ? 1.0 : 0.0);
            fl_st_f64<LDS>(&flow[x], 0.0);
            fl_st<LDS, depth_t>(&depth[x],
                                (depth_t)((px == 0 || px == kFailInf) ? 0 : Dp::kPending));
        }
        __syncthreads();

        // 3b. depth and sigma: sweep j finalises the vertices whose longest chain is j
        done = false;
        int top = 0;
        for (int j = 1; j <= V; ++j) {
            int pending = 0;
            for (int x = tid; x < V; x += kFailThreads) {
                if ((int)fl_ld<LDS, depth_t>(&depth[x]) != Dp::kPending) continue;
                const uint32_t px = fl_ld<LDS, uint32_t>(&pc[x]);
                double c = 0.0;
                bool any = false, ready = true;
                const int e0 = row_ptr[x], re = row_ptr[x + 1];
                FailCursor fc(fl_ld<LDS, uint8_t>(&flag[x]) != 0, fail, nfail, e0);
                for (int e = e0; e < re; ++e) {
                    if (fc.dead(e)) continue;
                    const int n = col[e];
                    const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[n]);
                    if (pn == kFailInf ||
                        (uint64_t)pn + (cost ? cost[e] : 1u) != (uint64_t)px)
                        continue;
                    if ((int)fl_ld<LDS, depth_t>(&depth[n]) >= j) {   // pending, or final in this sweep
                        ready = false;
                        break;
                    }
                    any = true;
                    c += hop ? 1.0 : fl_ld_f64<LDS>(&sigma[n]);
                }
                if (!ready) {
                    pending = 1;
                    continue;
                }
                // (no next hop cannot happen under our own pcost) dead next hops, overflow
                if (!(c > 0.0) || c > 1.7976931348623157e308) {
                    atomicOr(err, kErrFailureLoads);
                    c = 0.0;
                }
                fl_st_f64<LDS>(&sigma[x], c);
                fl_st<LDS, depth_t>(&depth[x], (depth_t)(any ? j : 0));
            }
            top = j;
            if (!__syncthreads_or(pending)) {
                done = true;
                break;
            }
        }
        if (!done) {                                       // (uniform) no DAG of V vertices does that
            if (tid == 0) atomicOr(err, kErrFailureLoads);
            continue;
        }

        // 4. the row's demand enters at its sources; 5. who is routed, what is lost
        double gone = 0.0;
        for (int64_t i = lo + tid; i < hi; i += kFailThreads) {
            const int s = srcs[i];
            if (s < 0 || s >= V) {
                if (rt) rt[i - pair_lo] = 0;
                continue;
            }
            const uint32_t ps = fl_ld<LDS, uint32_t>(&pc[s]);
            if (rt) rt[i - pair_lo] = ps != kFailInf;
            if (ps == 0) continue;                         // s == d
            const uint64_t w = weight ? weight[i] : 1ull;
            if (!w) continue;
            if (ps == kFailInf) gone += (double)w;
            else atomicAdd(&flow[s], (double)w);
        }
        if (lost && gone > 0.0) atomicAdd(&lost[k], gone);
        __syncthreads();

        //    push, deepest first
        double *out = load + (size_t)k * (size_t)E;
        for (int D = top; D >= 1; --D) {
            for (int x = tid; x < V; x += kFailThreads) {
                if ((int)fl_ld<LDS, depth_t>(&depth[x]) != D) continue;
                const double f = fl_ld_f64<LDS>(&flow[x]);
                const double sx = fl_ld_f64<LDS>(&sigma[x]);
                if (!(f > 0.0) || !(sx > 0.0)) continue;   // (sx == 0: reported in step 3)
                const uint32_t px = fl_ld<LDS, uint32_t>(&pc[x]);
                const int e0 = row_ptr[x], re = row_ptr[x + 1];
                FailCursor fc(fl_ld<LDS, uint8_t>(&flag[x]) != 0, fail, nfail, e0);
                for (int e = e0; e < re; ++e) {
                    if (fc.dead(e)) continue;              // tight or not: a dead link carries nothing
                    const int n = col[e];
                    const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[n]);
                    if (pn == kFailInf ||
                        (uint64_t)pn + (cost ? cost[e] : 1u) != (uint64_t)px)
                        continue;
                    // sigma[n] <= sigma[x]: the share is in [0, 1]
                    const double g = hop ? f / sx : f * (fl_ld_f64<LDS>(&sigma[n]) / sx);
                    if (!(g > 0.0)) continue;
                    if (pn != 0) atomicAdd(&flow[n], g);   // (pcost 0: the destination absorbs)
                    atomicAdd(&out[e], g);
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace

int sdnr_launch_failure_ecmp_link_loads(sdnr_ctx *ctx, const int32_t *d_dst, int32_t nrows,
                                        const int64_t *d_pair_off, int64_t pair_lo,
                                        int64_t pair_hi, const int32_t *d_srcs,
                                        const uint64_t *d_weight, int32_t nscen,
                                        const int64_t *d_scen_off, int64_t scen_lo,
                                        int64_t scen_hi, const int32_t *d_scen_edges,
                                        double *d_load, double *d_lost, uint8_t *d_routed,
                                        bool hop)
{
    const int V = ctx->V;
    const int64_t nitems = (int64_t)nscen * (int64_t)nrows;
    const uint32_t *cost = ctx->has_cost ? ctx->cost : nullptr;    // none: every link costs 1
    ctx->last_launches = 1;
    if (V <= kFailureLdsMaxV) {
        const size_t lds = ((size_t)V * kFailureBytesPerV + 15) & ~(size_t)15;
        auto fn = failure_ecmp_loads_kernel<true>;
        sdnr_allow_lds(reinterpret_cast<const void *>(fn), lds);
        int per_cu = (int)(SDNR_LDS_PER_CU / (lds ? lds : 1));
        per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);     // 2048 threads per CU
        int64_t g = (int64_t)ctx->num_cus * per_cu;
        if (g > nitems) g = nitems;
        ctx->last_kernel = "failure_ecmp_loads_kernel<lds>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kFailThreads), lds, ctx->stream, V, ctx->E,
                           nrows, nscen, hop ? 1 : 0, ctx->row_ptr, ctx->col, cost, d_dst,
                           d_pair_off, pair_lo, pair_hi, d_srcs, d_weight, d_scen_off, scen_lo,
                           scen_hi, d_scen_edges, d_load, d_lost, d_routed,
                           (unsigned char *)nullptr, (size_t)0, ctx->d_err);
    } else {
        // per workgroup: sigma, flow, pcost, u32 depths and the flags, 256-byte aligned
        const size_t stride = (((size_t)V * 25) + 255) & ~(size_t)255;
        int64_t g = (int64_t)ctx->num_cus * 2;
        if (g > nitems) g = nitems;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
        const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, stride * (size_t)g);
        if (rc) return rc;
        ctx->last_kernel = "failure_ecmp_loads_kernel<global>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(failure_ecmp_loads_kernel<false>, dim3((unsigned)g),
                           dim3(kFailThreads), 0, ctx->stream, V, ctx->E, nrows, nscen,
                           hop ? 1 : 0, ctx->row_ptr, ctx->col, cost, d_dst, d_pair_off, pair_lo,
                           pair_hi, d_srcs, d_weight, d_scen_off, scen_lo, scen_hi, d_scen_edges,
                           d_load, d_lost, d_routed, static_cast<unsigned char *>(ctx->scratch),
                           stride, ctx->d_err);
    }
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}
