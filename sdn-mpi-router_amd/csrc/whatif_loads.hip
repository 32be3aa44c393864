// whatif_loads.hip -- link-cost what-if loads: the ECMP-over-least-cost link
// loads of a traffic matrix once per COST scenario, the uploaded graph and
// costs untouched, and the peak utilisation of every scenario.
//
// A scenario is a list of cost overrides (CSR edge index, new cost), the edge
// indices strictly ascending.  The new cost SDNR_COST_INF takes the link down:
// failure_loads.hip's "this link is dead" is the special case "this link now
// costs INF".  A work item is (scenario k, destination row r), one workgroup
// persistent over the items, and the steps are failure_loads.hip's -- mask,
// pcost, order, push, reach, the row state in LDS from start to end -- with
// one difference: the merge cursor of a flagged vertex does not answer "is
// edge e dead" but "what does edge e cost in this scenario": its base cost
// (the uploaded one, 1 without uploaded costs), its override, or dead.
//   pcost   the pull Bellman-Ford adds the cost in force; a dead link is
//           skipped.  Every cost in force is >= 1 (an override of 0 is
//           refused), so "a vertex whose value is <= the number of sweeps
//           done is final" holds as it does there, for lowered costs too;
//   order   a link is a next-hop link when pcost[n] + the cost in force ==
//           pcost[x]; a dead link never is, tight by its base cost or not;
//   push    the same test: all three walks read the same cost, or flow
//           would be dropped between them.
// A vertex without the flag -- nearly all of them -- pays one integer compare
// per edge in the depth and push walks and nothing in the Bellman-Ford (the
// bare walk).
//
// Invalid entries.  An override is invalid when its cost is 0, or finite with
// cost * (V - 1) >= SDNR_COST_INF (sdnr_graph_costs' rule), when its index is
// outside [0, E), or when its index is not greater than its predecessor's.
// An invalid entry is ignored -- the link keeps the cost it had -- and
// reported.  The bisection of the cursor needs an ascending list: a scenario
// with an entry out of order (found in the mask step, a workgroup-uniform
// fact) is walked by a plain scan of the whole list per edge instead, which
// applies exactly the valid entries; that is the error path, its speed is of
// no interest.  Offsets outside their lists, sweeps that outrun V and a sigma
// above the double range are handled as in failure_loads.hip.  No NaN or Inf
// is ever formed.
//
// Row state: as failure_loads.hip (23 bytes per vertex in LDS up to
// kFailureLdsMaxV vertices, else 25 in the context scratch).
//
// whatif_peak_kernel, one workgroup per scenario, reduces a load slice to
// peak[k] = max over e of load[k][e] / capacity[e] and the smallest edge that
// attains it: a search over costs needs one number per candidate, not a plane.
#include "common.h"
#include "rowstate.h"

namespace {

constexpr int kWhatifThreads = 1024;
constexpr int kPeakThreads = 256;
constexpr uint32_t kWhatifInf = SDNR_COST_INF;
constexpr int kNoOverride = 0x7FFFFFFF;

// the upload's rule: cmax = the largest finite cost with cost * (V - 1) < INF
__device__ __forceinline__ bool whatif_cost_ok(uint32_t c, uint32_t cmax)
{
    return c == kWhatifInf || (c >= 1u && c <= cmax);
}

// The overrides of one scenario, edge[0 .. hi) ascending with their costs,
// seen from the row walk of one vertex.  cost(e, base): the cost of edge e in
// force -- e ascends along the walk, the cursor follows.
struct CostCursor {
    const int32_t *edge;
    const uint32_t *ncost;
    int hi, at, next;
    uint32_t cmax;
    bool scan;

    // flagged: the walk of a vertex with overridden out-links starts at its
    // first edge e0 -- the first entry >= e0 by bisection; else nothing ever
    // matches.  messy (a list out of order): every edge of a flagged vertex
    // scans the list
    __device__ __forceinline__ CostCursor(bool flagged, bool messy, const int32_t *f,
                                          const uint32_t *c, int n, int e0, uint32_t cm)
        : edge(f), ncost(c), hi(n), at(n), next(kNoOverride), cmax(cm), scan(flagged && messy)
    {
        if (!flagged || messy) return;
        int a = 0, b = n;
        while (a < b) {
            const int m = a + ((b - a) >> 1);
            if (f[m] < e0) a = m + 1;
            else b = m;
        }
        at = a;
        if (a < n) next = f[a];
    }
    __device__ __forceinline__ uint32_t cost(int e, uint32_t base)
    {
        if (scan) return scan_cost(e, base);
        if (e < next) return base;                         // (always, without the flag)
        uint32_t c = base;
        do {                                               // at <= hi: it ends
            if (next == e) {
                const uint32_t o = ncost[at];
                if (whatif_cost_ok(o, cmax)) c = o;         // (strictly ascending: one match)
            }
            ++at;
            next = at < hi ? edge[at] : kNoOverride;
        } while (next <= e);
        return c;
    }
    // the error path: the valid entries of a list that is not ascending
    __device__ __forceinline__ uint32_t scan_cost(int e, uint32_t base) const
    {
        uint32_t c = base;
        for (int i = 0; i < hi; ++i) {
            if (edge[i] != e || (i > 0 && edge[i - 1] >= e)) continue;
            const uint32_t o = ncost[i];
            if (whatif_cost_ok(o, cmax)) c = o;
        }
        return c;
    }
};

// hop: sigma[x] holds the number of next hops instead of the route count
template <bool LDS>
__global__ __launch_bounds__(kWhatifThreads) void whatif_ecmp_loads_kernel(
    int V, int E, int nrows, int nscen, int hop, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const uint32_t *__restrict__ cost,
    const int32_t *__restrict__ dst, const int64_t *__restrict__ pair_off, int64_t pair_lo,
    int64_t pair_hi, const int32_t *__restrict__ srcs, const uint64_t *__restrict__ weight,
    const int64_t *__restrict__ scen_off, int64_t scen_lo, int64_t scen_hi,
    const int32_t *__restrict__ scen_edges, const uint32_t *__restrict__ scen_costs,
    double *__restrict__ load, double *__restrict__ lost, unsigned char *__restrict__ routed,
    unsigned char *__restrict__ scratch, size_t scratch_stride, int *__restrict__ err)
{
    typedef FailDepth<LDS> Dp;
    typedef typename Dp::T depth_t;
    // sigma f64 [V] | flow f64 [V] | pcost u32 [V] | depth u16 / u32 [V] | flag u8 [V]
    extern __shared__ __attribute__((aligned(16))) unsigned char whatif_lds[];
    unsigned char *base = LDS ? whatif_lds : scratch + (size_t)blockIdx.x * scratch_stride;
    double *sigma = reinterpret_cast<double *>(base);
    double *flow = sigma + V;
    uint32_t *pc = reinterpret_cast<uint32_t *>(flow + V);
    depth_t *depth = reinterpret_cast<depth_t *>(pc + V);
    uint8_t *flag = reinterpret_cast<uint8_t *>(depth + V);
    const int tid = (int)threadIdx.x;
    const int64_t npairs = pair_hi - pair_lo;
    const int64_t nitems = (int64_t)nscen * (int64_t)nrows;
    const uint32_t cmax = V > 1 ? (kWhatifInf - 1u) / (uint32_t)(V - 1) : kWhatifInf - 1u;

    for (int64_t item = (int64_t)blockIdx.x; item < nitems; item += (int64_t)gridDim.x) {
        const int k = (int)(item / nrows), r = (int)(item % nrows);
        const int64_t lo = pair_off[r], hi = pair_off[r + 1];
        if (lo < pair_lo || hi > pair_hi || hi < lo) {     // offsets outside the pair list
            if (tid == 0) atomicOr(err, kErrWhatifLoads);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no demand)
        const int64_t flo64 = scen_off[k], fhi64 = scen_off[k + 1];
        if (flo64 < scen_lo || fhi64 > scen_hi || fhi64 < flo64 ||
            fhi64 - flo64 > (int64_t)0x7FFFFFF0) {         // ... outside the scenario list
            if (tid == 0) atomicOr(err, kErrWhatifLoads);
            continue;
        }
        const int32_t *ovr = scen_edges + flo64;           // (never read when novr == 0)
        const uint32_t *ovc = scen_costs + flo64;
        const int novr = (int)(fhi64 - flo64);
        int d = dst[r];
        if (d < 0 || d >= V) d = -1;                       // no vertex: an empty row
        // routed[k][i - pair_lo]
        unsigned char *rt = routed ? routed + (size_t)k * (size_t)npairs : nullptr;

        if (d < 0) {                                       // (uniform) nothing routed, all lost
            double gone = 0.0;
            for (int64_t i = lo + tid; i < hi; i += kWhatifThreads) {
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
        for (int x = tid; x < V; x += kWhatifThreads) {
            fl_st<LDS, uint32_t>(&pc[x], x == d ? 0u : kWhatifInf);
            fl_st<LDS, uint8_t>(&flag[x], (uint8_t)0);
        }
        __syncthreads();
        //    ... flag the source vertex of every overridden link
        int disorder = 0;
        for (int i = tid; i < novr; i += kWhatifThreads) {
            const int f = ovr[i];
            bool bad = !whatif_cost_ok(ovc[i], cmax);      // a cost the upload refuses
            if (i > 0 && ovr[i - 1] >= f) {                // not strictly ascending
                bad = true;
                disorder = 1;
            }
            if (f < 0 || f >= E) bad = true;               // no link
            if (bad) atomicOr(err, kErrWhatifLoads);       // ignored (by the cursor), reported
            if (f < 0 || f >= E) continue;
            int a = 0, b = V;                              // the x with row_ptr[x] <= f < row_ptr[x + 1]
            while (b - a > 1) {
                const int m = a + ((b - a) >> 1);
                if (row_ptr[m] <= f) a = m;
                else b = m;
            }
            fl_st<LDS, uint8_t>(&flag[a], (uint8_t)1);
        }
        const bool messy = __syncthreads_or(disorder) != 0;

        // 2. least costs: sweeps until one changes nothing
        bool done = false;
        for (int sweep = 0; sweep < V; ++sweep) {
            int changed = 0;
            for (int x = tid; x < V; x += kWhatifThreads) {
                const uint32_t cur = fl_ld<LDS, uint32_t>(&pc[x]);
                // costs in force are >= 1: a route of cost <= sweep has <= sweep links, and
                // after `sweep` sweeps every vertex with such a least-cost route is final
                if (cur <= (uint32_t)sweep) continue;
                uint32_t best = cur;
                const int e0 = row_ptr[x], re = row_ptr[x + 1];
                // t > pn: pn is finite (INF + c wraps) and the sum did not wrap
                if (!fl_ld<LDS, uint8_t>(&flag[x])) {       // nearly every vertex: the bare walk
#pragma unroll 4
                    for (int e = e0; e < re; ++e) {
                        const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[col[e]]);
                        const uint32_t t = pn + (cost ? cost[e] : 1u);
                        if (t > pn && t < best) best = t;
                    }
                } else {
                    CostCursor cc(true, messy, ovr, ovc, novr, e0, cmax);
                    for (int e = e0; e < re; ++e) {
                        const uint32_t c = cc.cost(e, cost ? cost[e] : 1u);
                        if (c == kWhatifInf) continue;     // down
                        const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[col[e]]);
                        const uint32_t t = pn + c;
                        if (t > pn && t < best) best = t;
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
            if (tid == 0) atomicOr(err, kErrWhatifLoads);
            continue;
        }

        // 3a. flow = 0; the destination and the unreachable are final at depth 0
        for (int x = tid; x < V; x += kWhatifThreads) {
            const uint32_t px = fl_ld<LDS, uint32_t>(&pc[x]);
            fl_st_f64<LDS>(&sigma[x], (px == 0 && !hop) ? 1.0 : 0.0);
            fl_st_f64<LDS>(&flow[x], 0.0);
            fl_st<LDS, depth_t>(&depth[x],
                                (depth_t)((px == 0 || px == kWhatifInf) ? 0 : Dp::kPending));
        }
        __syncthreads();

        // 3b. depth and sigma: sweep j finalises the vertices whose longest chain is j
        done = false;
        int top = 0;
        for (int j = 1; j <= V; ++j) {
            int pending = 0;
            for (int x = tid; x < V; x += kWhatifThreads) {
                if ((int)fl_ld<LDS, depth_t>(&depth[x]) != Dp::kPending) continue;
                const uint32_t px = fl_ld<LDS, uint32_t>(&pc[x]);
                double c = 0.0;
                bool any = false, ready = true;
                const int e0 = row_ptr[x], re = row_ptr[x + 1];
                CostCursor cc(fl_ld<LDS, uint8_t>(&flag[x]) != 0, messy, ovr, ovc, novr, e0, cmax);
                for (int e = e0; e < re; ++e) {
                    const uint32_t ce = cc.cost(e, cost ? cost[e] : 1u);
                    if (ce == kWhatifInf) continue;
                    const int n = col[e];
                    const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[n]);
                    if (pn == kWhatifInf || (uint64_t)pn + ce != (uint64_t)px) continue;
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
                    atomicOr(err, kErrWhatifLoads);
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
            if (tid == 0) atomicOr(err, kErrWhatifLoads);
            continue;
        }

        // 4. the row's demand enters at its sources; 5. who is routed, what is lost
        double gone = 0.0;
        for (int64_t i = lo + tid; i < hi; i += kWhatifThreads) {
            const int s = srcs[i];
            if (s < 0 || s >= V) {
                if (rt) rt[i - pair_lo] = 0;
                continue;
            }
            const uint32_t ps = fl_ld<LDS, uint32_t>(&pc[s]);
            if (rt) rt[i - pair_lo] = ps != kWhatifInf;
            if (ps == 0) continue;                         // s == d
            const uint64_t w = weight ? weight[i] : 1ull;
            if (!w) continue;
            if (ps == kWhatifInf) gone += (double)w;
            else atomicAdd(&flow[s], (double)w);
        }
        if (lost && gone > 0.0) atomicAdd(&lost[k], gone);
        __syncthreads();

        //    push, deepest first
        double *out = load + (size_t)k * (size_t)E;
        for (int D = top; D >= 1; --D) {
            for (int x = tid; x < V; x += kWhatifThreads) {
                if ((int)fl_ld<LDS, depth_t>(&depth[x]) != D) continue;
                const double f = fl_ld_f64<LDS>(&flow[x]);
                const double sx = fl_ld_f64<LDS>(&sigma[x]);
                if (!(f > 0.0) || !(sx > 0.0)) continue;   // (sx == 0: reported in step 3)
                const uint32_t px = fl_ld<LDS, uint32_t>(&pc[x]);
                const int e0 = row_ptr[x], re = row_ptr[x + 1];
                CostCursor cc(fl_ld<LDS, uint8_t>(&flag[x]) != 0, messy, ovr, ovc, novr, e0, cmax);
                for (int e = e0; e < re; ++e) {
                    const uint32_t ce = cc.cost(e, cost ? cost[e] : 1u);
                    if (ce == kWhatifInf) continue;        // tight or not: a dead link carries nothing
                    const int n = col[e];
                    const uint32_t pn = fl_ld<LDS, uint32_t>(&pc[n]);
                    if (pn == kWhatifInf || (uint64_t)pn + ce != (uint64_t)px) continue;
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

// (u, e) orders before (v, f): the larger utilisation, then the smaller edge
__device__ __forceinline__ bool peak_before(double u, int e, double v, int f)
{
    return u > v || (u == v && e < f);
}

// peak[k] = max over e of load[k][e] / capacity[e] (capacity NULL: 1.0 each),
// peak_edge[k] = the smallest e attaining it; 0.0 and -1 when no link carries
// anything.  Loads are >= 0 and finite (what the kernels above add).
__global__ __launch_bounds__(kPeakThreads) void whatif_peak_kernel(
    int E, const double *__restrict__ load, const double *__restrict__ capacity,
    double *__restrict__ peak, int32_t *__restrict__ peak_edge, int *__restrict__ err)
{
    __shared__ double wave_u[kPeakThreads / SDNR_WAVE];
    __shared__ int wave_e[kPeakThreads / SDNR_WAVE];
    const int k = (int)blockIdx.x, tid = (int)threadIdx.x;
    const double *row = load + (size_t)k * (size_t)E;
    double bu = 0.0;
    int be = -1;
    for (int e = tid; e < E; e += kPeakThreads) {          // e ascends: a tie keeps the first
        double u = row[e];
        if (capacity) {
            const double c = capacity[e];
            if (!(c > 0.0) || c > 1.7976931348623157e308) {    // zero, negative, NaN, Inf
                atomicOr(err, kErrWhatifLoads);
                continue;
            }
            u = u / c;
        }
        if (u > bu) {
            bu = u;
            be = e;
        }
    }
    // (be == -1 goes with bu == 0.0 and only then: equal utilisations above 0
    // compare real edges, two empty hands compare -1 with -1)
    for (int s = SDNR_WAVE / 2; s >= 1; s >>= 1) {
        const double ou = __shfl_down(bu, s);
        const int oe = __shfl_down(be, s);
        if (peak_before(ou, oe, bu, be) && oe >= 0) {
            bu = ou;
            be = oe;
        }
    }
    if ((tid & (SDNR_WAVE - 1)) == 0) {
        wave_u[tid / SDNR_WAVE] = bu;
        wave_e[tid / SDNR_WAVE] = be;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kPeakThreads / SDNR_WAVE; ++w)
            if (wave_e[w] >= 0 && peak_before(wave_u[w], wave_e[w], bu, be)) {
                bu = wave_u[w];
                be = wave_e[w];
            }
        peak[k] = bu;
        peak_edge[k] = be;
    }
}

}  // namespace

int sdnr_launch_whatif_ecmp_link_loads(sdnr_ctx *ctx, const int32_t *d_dst, int32_t nrows,
                                       const int64_t *d_pair_off, int64_t pair_lo,
                                       int64_t pair_hi, const int32_t *d_srcs,
                                       const uint64_t *d_weight, int32_t nscen,
                                       const int64_t *d_scen_off, int64_t scen_lo,
                                       int64_t scen_hi, const int32_t *d_scen_edges,
                                       const uint32_t *d_scen_costs, double *d_load,
                                       double *d_lost, uint8_t *d_routed, bool hop)
{
    const int V = ctx->V;
    const int64_t nitems = (int64_t)nscen * (int64_t)nrows;
    const uint32_t *cost = ctx->has_cost ? ctx->cost : nullptr;    // none: every link costs 1
    ctx->last_launches = 1;
    if (V <= kFailureLdsMaxV) {
        const size_t lds = ((size_t)V * kFailureBytesPerV + 15) & ~(size_t)15;
        auto fn = whatif_ecmp_loads_kernel<true>;
        sdnr_allow_lds(reinterpret_cast<const void *>(fn), lds);
        int per_cu = (int)(SDNR_LDS_PER_CU / (lds ? lds : 1));
        per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);     // 2048 threads per CU
        int64_t g = (int64_t)ctx->num_cus * per_cu;
        if (g > nitems) g = nitems;
        ctx->last_kernel = "whatif_ecmp_loads_kernel<lds>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kWhatifThreads), lds, ctx->stream, V,
                           ctx->E, nrows, nscen, hop ? 1 : 0, ctx->row_ptr, ctx->col, cost, d_dst,
                           d_pair_off, pair_lo, pair_hi, d_srcs, d_weight, d_scen_off, scen_lo,
                           scen_hi, d_scen_edges, d_scen_costs, d_load, d_lost, d_routed,
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
        ctx->last_kernel = "whatif_ecmp_loads_kernel<global>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(whatif_ecmp_loads_kernel<false>, dim3((unsigned)g),
                           dim3(kWhatifThreads), 0, ctx->stream, V, ctx->E, nrows, nscen,
                           hop ? 1 : 0, ctx->row_ptr, ctx->col, cost, d_dst, d_pair_off, pair_lo,
                           pair_hi, d_srcs, d_weight, d_scen_off, scen_lo, scen_hi, d_scen_edges,
                           d_scen_costs, d_load, d_lost, d_routed,
                           static_cast<unsigned char *>(ctx->scratch), stride, ctx->d_err);
    }
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}

int sdnr_launch_whatif_peak(sdnr_ctx *ctx, int32_t nscen, const double *d_load,
                            const double *d_capacity, double *d_peak, int32_t *d_peak_edge)
{
    hipLaunchKernelGGL(whatif_peak_kernel, dim3((unsigned)nscen), dim3(kPeakThreads), 0,
                       ctx->stream, ctx->E, d_load, d_capacity, d_peak, d_peak_edge, ctx->d_err);
    SDNR_HIP(hipGetLastError());
    return SDNR_OK;
}
