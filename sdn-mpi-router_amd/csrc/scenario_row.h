// scenario_row.h -- the one body of the fused what-if kernels and their one
// launcher: failure_loads.hip and whatif_loads.hip instantiate it with their
// Scenario policy.  Their file headers say what the steps compute and why; the
// text of the steps is here.
//
// A Scenario holds the scenario lists of a call and provides
//   kErr                      the bit it raises in the context's error word;
//   list(lo, n)               the Scenario of one list, entries [lo, lo + n);
//   edge(i)                   the CSR edge index of entry i of that list;
//   check(i, E, err)          reports entry i if it is invalid (it is ignored
//                             by the cursor) and returns 1 if it breaks the
//                             order that the cursor's bisection needs;
//   settle(disorder)          the barrier that ends the mask step, and the
//                             workgroup-uniform `messy`: some thread saw
//                             disorder (constant false where none can);
//   reaches(pn, t)            the guard of the Bellman-Ford walks: pn is
//                             finite, so t = pn + cost is a route's cost;
//   cursor(flagged, messy, e0)  the list seen from the row walk of a vertex
//                             whose edges start at e0, with
//       live(e, cost, c)      is edge e up in this scenario (cost: the
//                             uploaded costs, NULL when every link costs 1);
//                             it may leave the cost in force in c.  e ascends
//                             along the walk, one call per edge.  Without
//                             the flag it costs one integer compare;
//       cost(e, cost, c)      the cost in force of the edge live() just said
//                             is up, c as live() left it: a policy reads the
//                             base cost in the one of the two that needs it
//                             first.
// All three walks of an item (pcost, order, push) read the same cursor, or
// flow would be dropped between them; the Bellman-Ford walk of a vertex
// without the flag reads none (the bare walk).
#pragma once

#include "common.h"
#include "rowstate.h"

// chains of dependent LDS / L2 reads per thread (as cost_tables.hip and
// cost_ecmp_loads.hip): the waves that hide them come from the workgroup
constexpr int kScenarioThreads = 1024;

// hop: sigma[x] holds the number of next hops instead of the route count
template <bool LDS, class Scenario>
__device__ __forceinline__ void scenario_row_body(
    const Scenario all, int V, int E, int nrows, int nscen, int hop,
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const uint32_t *__restrict__ cost, const int32_t *__restrict__ dst,
    const int64_t *__restrict__ pair_off, int64_t pair_lo, int64_t pair_hi,
    const int32_t *__restrict__ srcs, const uint64_t *__restrict__ weight,
    const int64_t *__restrict__ scen_off, int64_t scen_lo, int64_t scen_hi,
    double *__restrict__ load, double *__restrict__ lost, unsigned char *__restrict__ routed,
    unsigned char *__restrict__ scratch, size_t scratch_stride, int *__restrict__ err)
{
    typedef FailDepth<LDS> Dp;
    typedef typename Dp::T depth_t;
    typedef typename Scenario::Cursor Cursor;
    constexpr uint32_t kInf = SDNR_COST_INF;
    constexpr int kErr = Scenario::kErr;
    // sigma f64 [V] | flow f64 [V] | pcost u32 [V] | depth u16 / u32 [V] | flag u8 [V]
    extern __shared__ __attribute__((aligned(16))) unsigned char scenario_lds[];
    unsigned char *base = LDS ? scenario_lds : scratch + (size_t)blockIdx.x * scratch_stride;
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
            if (tid == 0) atomicOr(err, kErr);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no demand)
        const int64_t flo64 = scen_off[k], fhi64 = scen_off[k + 1];
        if (flo64 < scen_lo || fhi64 > scen_hi || fhi64 < flo64 ||
            fhi64 - flo64 > (int64_t)0x7FFFFFF0) {         // ... outside the scenario list
            if (tid == 0) atomicOr(err, kErr);
            continue;
        }
        const int nent = (int)(fhi64 - flo64);
        const Scenario sc = all.list(flo64, nent);         // (never read when nent == 0)
        int d = dst[r];
        if (d < 0 || d >= V) d = -1;                       // no vertex: an empty row
        // routed[k][i - pair_lo]
        unsigned char *rt = routed ? routed + (size_t)k * (size_t)npairs : nullptr;

        if (d < 0) {                                       // (uniform) nothing routed, all lost
            double gone = 0.0;
            for (int64_t i = lo + tid; i < hi; i += kScenarioThreads) {
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
        for (int x = tid; x < V; x += kScenarioThreads) {
            fl_st<LDS, uint32_t>(&pc[x], x == d ? 0u : kInf);
            fl_st<LDS, uint8_t>(&flag[x], (uint8_t)0);
        }
        __syncthreads();
        //    ... flag the source vertex of every listed link
        int disorder = 0;
        for (int i = tid; i < nent; i += kScenarioThreads) {
            const int f = sc.edge(i);
            disorder |= sc.check(i, E, err);
            if (f < 0 || f >= E) continue;                 // no link
            int a = 0, b = V;                              // the x with row_ptr[x] <= f < row_ptr[x + 1]
            while (b - a > 1) {
                const int m = a + ((b - a) >> 1);
                if (row_ptr[m] <= f) a = m;
                else b = m;
            }
            fl_st<LDS, uint8_t>(&flag[a], (uint8_t)1);
        }
        const bool messy = Scenario::settle(disorder);

        // 2. least costs: sweeps until one changes nothing
        bool done = false;
        for (int sweep = 0; sweep < V; ++sweep) {
            int changed = 0;
            for (int x = tid; x < V; x += kScenarioThreads) {
                const uint32_t cur = fl_ld<LDS, uint32_t>(&pc[x]);
                // costs in force are >= 1: a route of cost <= sweep has <= sweep links, and
                // after `sweep` sweeps every vertex with such a least-cost route is final
                if (cur <= (uint32_t)sweep) continue;
                uint32_t best = cur;
                const int e0 = row_ptr[x], re = row_ptr[x + 1];
                if (!fl_ld<LDS, uint8_t>(&flag[x])) {       // nearly every vertex: the bare walk
#pragma unroll 4
                    for (int e = e0; e < re; ++e) {
                        const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[col[e]]);
                        const uint32_t t = pn + (cost ? cost[e] : 1u);   // (unused when pn is INF)
                        if (Scenario::reaches(pn, t) && t < best) best = t;
                    }
                } else {
                    Cursor cu = sc.cursor(true, messy, e0);
                    for (int e = e0; e < re; ++e) {
                        uint32_t ce;
                        if (!cu.live(e, cost, ce)) continue;
                        const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[col[e]]);
                        const uint32_t t = pn + cu.cost(e, cost, ce);
                        if (Scenario::reaches(pn, t) && t < best) best = t;
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
            if (tid == 0) atomicOr(err, kErr);
            continue;
        }

        // 3a. flow = 0; the destination and the unreachable are final at depth 0
        for (int x = tid; x < V; x += kScenarioThreads) {
            const uint32_t px = fl_ld<LDS, uint32_t>(&pc[x]);
            fl_st_f64<LDS>(&sigma[x], (px == 0 && !hop) ? 1.0 : 0.0);
            fl_st_f64<LDS>(&flow[x], 0.0);
            fl_st<LDS, depth_t>(&depth[x], (depth_t)((px == 0 || px == kInf) ? 0 : Dp::kPending));
        }
        __syncthreads();

        // 3b. depth and sigma: sweep j finalises the vertices whose longest chain is j
        done = false;
        int top = 0;
        for (int j = 1; j <= V; ++j) {
            int pending = 0;
            for (int x = tid; x < V; x += kScenarioThreads) {
                if ((int)fl_ld<LDS, depth_t>(&depth[x]) != Dp::kPending) continue;
                const uint32_t px = fl_ld<LDS, uint32_t>(&pc[x]);
                double c = 0.0;
                bool any = false, ready = true;
                const int e0 = row_ptr[x], re = row_ptr[x + 1];
                Cursor cu = sc.cursor(fl_ld<LDS, uint8_t>(&flag[x]) != 0, messy, e0);
                for (int e = e0; e < re; ++e) {
                    uint32_t ce;
                    if (!cu.live(e, cost, ce)) continue;
                    const int n = col[e];
                    const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[n]);
                    if (pn == kInf || (uint64_t)pn + cu.cost(e, cost, ce) != (uint64_t)px) continue;
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
                    atomicOr(err, kErr);
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
            if (tid == 0) atomicOr(err, kErr);
            continue;
        }

        // 4. the row's demand enters at its sources; 5. who is routed, what is lost
        double gone = 0.0;
        for (int64_t i = lo + tid; i < hi; i += kScenarioThreads) {
            const int s = srcs[i];
            if (s < 0 || s >= V) {
                if (rt) rt[i - pair_lo] = 0;
                continue;
            }
            const uint32_t ps = fl_ld<LDS, uint32_t>(&pc[s]);
            if (rt) rt[i - pair_lo] = ps != kInf;
            if (ps == 0) continue;                         // s == d
            const uint64_t w = weight ? weight[i] : 1ull;
            if (!w) continue;
            if (ps == kInf) gone += (double)w;
            else atomicAdd(&flow[s], (double)w);
        }
        if (lost && gone > 0.0) atomicAdd(&lost[k], gone);
        __syncthreads();

        //    push, deepest first
        double *out = load + (size_t)k * (size_t)E;
        for (int D = top; D >= 1; --D) {
            for (int x = tid; x < V; x += kScenarioThreads) {
                if ((int)fl_ld<LDS, depth_t>(&depth[x]) != D) continue;
                const double f = fl_ld_f64<LDS>(&flow[x]);
                const double sx = fl_ld_f64<LDS>(&sigma[x]);
                if (!(f > 0.0) || !(sx > 0.0)) continue;   // (sx == 0: reported in step 3)
                const uint32_t px = fl_ld<LDS, uint32_t>(&pc[x]);
                const int e0 = row_ptr[x], re = row_ptr[x + 1];
                Cursor cu = sc.cursor(fl_ld<LDS, uint8_t>(&flag[x]) != 0, messy, e0);
                for (int e = e0; e < re; ++e) {
                    uint32_t ce;
                    if (!cu.live(e, cost, ce)) continue;   // tight or not: a dead link carries none
                    const int n = col[e];
                    const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[n]);
                    if (pn == kInf || (uint64_t)pn + cu.cost(e, cost, ce) != (uint64_t)px) continue;
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

// Launch lds_fn with the row state in LDS (V <= kFailureLdsMaxV), else
// global_fn with a slice of the context scratch per workgroup.  args: the
// kernel's parameters up to the three both kernels end in (scratch, its
// stride, the error word), which are added here.
template <class Fn, class... Args>
int scenario_launch(sdnr_ctx *ctx, int64_t nitems, Fn lds_fn, Fn global_fn, const char *lds_name,
                    const char *global_name, Args... args)
{
    const int V = ctx->V;
    const bool in_lds = V <= kFailureLdsMaxV;
    const Fn fn = in_lds ? lds_fn : global_fn;
    size_t lds = 0, stride = 0;
    int64_t g = (int64_t)ctx->num_cus * 2;                 // 2048 threads per CU
    ctx->last_launches = 1;
    if (in_lds) {
        lds = ((size_t)V * kFailureBytesPerV + 15) & ~(size_t)15;
        sdnr_allow_lds(reinterpret_cast<const void *>(fn), lds);
        if (lds * 2 > SDNR_LDS_PER_CU) g = ctx->num_cus;  // one workgroup's state fills the LDS
        if (g > nitems) g = nitems;
    } else {
        // per workgroup: sigma, flow, pcost, u32 depths and the flags, 256-byte aligned
        stride = (((size_t)V * 25) + 255) & ~(size_t)255;
        if (g > nitems) g = nitems;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
        const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, stride * (size_t)g);
        if (rc) return rc;
    }
    ctx->last_kernel = in_lds ? lds_name : global_name;
    ctx->last_grid = g;
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    unsigned char *scratch = in_lds ? nullptr : static_cast<unsigned char *>(ctx->scratch);
    hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kScenarioThreads), lds, ctx->stream, args...,
                       scratch, stride, ctx->d_err);
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}
