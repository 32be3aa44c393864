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
//
// The steps themselves are scenario_row.h's body, shared with failure_loads.hip;
// this file is its cost policy and the peak reduction.
#include "scenario_row.h"

namespace {

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
    // the shared body's pair: the cost in force is worked out once per edge
    __device__ __forceinline__ bool live(int e, const uint32_t *base, uint32_t &c)
    {
        c = cost(e, base ? base[e] : 1u);
        return c != kWhatifInf;                            // INF: down
    }
    __device__ __forceinline__ uint32_t cost(int, const uint32_t *, uint32_t c) const
    {
        return c;
    }
};

// scenario_row.h's policy: a list of (edge, new cost), the edges strictly ascending
struct CostScenario {
    typedef CostCursor Cursor;
    static constexpr int kErr = kErrWhatifLoads;
    const int32_t *ovr;
    const uint32_t *ovc;
    int n;
    uint32_t cmax;

    __device__ __forceinline__ CostScenario list(int64_t lo, int count) const
    {
        return CostScenario{ovr + lo, ovc + lo, count, cmax};
    }
    __device__ __forceinline__ int edge(int i) const { return ovr[i]; }
    __device__ __forceinline__ int check(int i, int E, int *err) const
    {
        const int f = ovr[i];
        bool bad = !whatif_cost_ok(ovc[i], cmax);          // a cost the upload refuses
        int disorder = 0;
        if (i > 0 && ovr[i - 1] >= f) {                    // not strictly ascending
            bad = true;
            disorder = 1;
        }
        if (f < 0 || f >= E) bad = true;                   // no link
        if (bad) atomicOr(err, kErr);                      // ignored (by the cursor), reported
        return disorder;
    }
    static __device__ __forceinline__ bool settle(int disorder)
    {
        return __syncthreads_or(disorder) != 0;
    }
    // t > pn: pn is finite (INF + c wraps) and the sum did not wrap
    static __device__ __forceinline__ bool reaches(uint32_t pn, uint32_t t) { return t > pn; }
    __device__ __forceinline__ Cursor cursor(bool flagged, bool messy, int e0) const
    {
        return Cursor(flagged, messy, ovr, ovc, n, e0, cmax);
    }
};

template <bool LDS>
__global__ __launch_bounds__(kScenarioThreads) void whatif_ecmp_loads_kernel(
    int V, int E, int nrows, int nscen, int hop, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const uint32_t *__restrict__ cost,
    const int32_t *__restrict__ dst, const int64_t *__restrict__ pair_off, int64_t pair_lo,
    int64_t pair_hi, const int32_t *__restrict__ srcs, const uint64_t *__restrict__ weight,
    const int64_t *__restrict__ scen_off, int64_t scen_lo, int64_t scen_hi,
    const int32_t *__restrict__ scen_edges, const uint32_t *__restrict__ scen_costs,
    double *__restrict__ load, double *__restrict__ lost, unsigned char *__restrict__ routed,
    unsigned char *__restrict__ scratch, size_t scratch_stride, int *__restrict__ err)
{
    const uint32_t cmax = V > 1 ? (kWhatifInf - 1u) / (uint32_t)(V - 1) : kWhatifInf - 1u;
    scenario_row_body<LDS>(CostScenario{scen_edges, scen_costs, 0, cmax}, V, E, nrows, nscen, hop,
                           row_ptr, col, cost, dst, pair_off, pair_lo, pair_hi, srcs, weight,
                           scen_off, scen_lo, scen_hi, load, lost, routed, scratch,
                           scratch_stride, err);
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
    const uint32_t *cost = ctx->has_cost ? ctx->cost : nullptr;    // none: every link costs 1
    return scenario_launch(ctx, (int64_t)nscen * (int64_t)nrows, whatif_ecmp_loads_kernel<true>,
                           whatif_ecmp_loads_kernel<false>, "whatif_ecmp_loads_kernel<lds>",
                           "whatif_ecmp_loads_kernel<global>", ctx->V, ctx->E, nrows, nscen,
                           hop ? 1 : 0, ctx->row_ptr, ctx->col, cost, d_dst, d_pair_off, pair_lo,
                           pair_hi, d_srcs, d_weight, d_scen_off, scen_lo, scen_hi, d_scen_edges,
                           d_scen_costs, d_load, d_lost, d_routed);
}

int sdnr_launch_whatif_peak(sdnr_ctx *ctx, int32_t nscen, const double *d_load,
                            const double *d_capacity, double *d_peak, int32_t *d_peak_edge)
{
    hipLaunchKernelGGL(whatif_peak_kernel, dim3((unsigned)nscen), dim3(kPeakThreads), 0,
                       ctx->stream, ctx->E, d_load, d_capacity, d_peak, d_peak_edge, ctx->d_err);
    SDNR_HIP(hipGetLastError());
    return SDNR_OK;
}
