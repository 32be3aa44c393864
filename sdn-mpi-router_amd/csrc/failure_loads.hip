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
//
// The steps themselves are scenario_row.h's body, shared with whatif_loads.hip;
// this file is its failure policy.
#include "scenario_row.h"

namespace {

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
    __device__ __forceinline__ bool live(int e, const uint32_t *, uint32_t &)
    {
        return !dead(e);
    }
    // a failure changes no cost: the base cost, read where the walk needs it
    __device__ __forceinline__ uint32_t cost(int e, const uint32_t *base, uint32_t) const
    {
        return base ? base[e] : 1u;
    }
};

// scenario_row.h's policy: a list of failed links, ascending, duplicates allowed
struct FailureScenario {
    typedef FailCursor Cursor;
    static constexpr int kErr = kErrFailureLoads;
    const int32_t *fail;
    int n;

    __device__ __forceinline__ FailureScenario list(int64_t lo, int count) const
    {
        return FailureScenario{fail + lo, count};
    }
    __device__ __forceinline__ int edge(int i) const { return fail[i]; }
    __device__ __forceinline__ int check(int i, int E, int *err) const
    {
        const int f = fail[i];
        if (i > 0 && fail[i - 1] > f) atomicOr(err, kErr);     // not ascending
        if (f < 0 || f >= E) atomicOr(err, kErr);              // no link: ignored, reported
        return 0;                                          // (the merge takes any ascending list)
    }
    static __device__ __forceinline__ bool settle(int)
    {
        __syncthreads();
        return false;
    }
    static __device__ __forceinline__ bool reaches(uint32_t pn, uint32_t)
    {
        return pn != SDNR_COST_INF;
    }
    __device__ __forceinline__ Cursor cursor(bool flagged, bool, int e0) const
    {
        return Cursor(flagged, fail, n, e0);
    }
};

template <bool LDS>
__global__ __launch_bounds__(kScenarioThreads) void failure_ecmp_loads_kernel(
    int V, int E, int nrows, int nscen, int hop, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const uint32_t *__restrict__ cost,
    const int32_t *__restrict__ dst, const int64_t *__restrict__ pair_off, int64_t pair_lo,
    int64_t pair_hi, const int32_t *__restrict__ srcs, const uint64_t *__restrict__ weight,
    const int64_t *__restrict__ scen_off, int64_t scen_lo, int64_t scen_hi,
    const int32_t *__restrict__ scen_edges, double *__restrict__ load, double *__restrict__ lost,
    unsigned char *__restrict__ routed, unsigned char *__restrict__ scratch,
    size_t scratch_stride, int *__restrict__ err)
{
    scenario_row_body<LDS>(FailureScenario{scen_edges, 0}, V, E, nrows, nscen, hop, row_ptr, col,
                           cost, dst, pair_off, pair_lo, pair_hi, srcs, weight, scen_off, scen_lo,
                           scen_hi, load, lost, routed, scratch, scratch_stride, err);
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
    const uint32_t *cost = ctx->has_cost ? ctx->cost : nullptr;    // none: every link costs 1
    return scenario_launch(ctx, (int64_t)nscen * (int64_t)nrows, failure_ecmp_loads_kernel<true>,
                           failure_ecmp_loads_kernel<false>, "failure_ecmp_loads_kernel<lds>",
                           "failure_ecmp_loads_kernel<global>", ctx->V, ctx->E, nrows, nscen,
                           hop ? 1 : 0, ctx->row_ptr, ctx->col, cost, d_dst, d_pair_off, pair_lo,
                           pair_hi, d_srcs, d_weight, d_scen_off, scen_lo, scen_hi, d_scen_edges,
                           d_load, d_lost, d_routed);
}
