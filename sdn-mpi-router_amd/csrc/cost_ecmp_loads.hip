// cost_ecmp_loads.hip -- per-link loads of a traffic matrix split over EVERY
// least-cost route (ECMP under per-link costs), where ecmp_loads.hip splits
// over the hop-count routes and loads.hip + cost_tables.hip put a pair on one.
//
// For a destination row d, pcost[x] is the least path cost from x to d
// (sdnr_cost_tables; SDNR_COST_INF: no route) and link e = (x -> n) is a
// next-hop link of x when pcost[n] != INF and pcost[n] + cost[e] == pcost[x].
// Costs are >= 1, so pcost strictly decreases along a next-hop link: the links
// form a DAG toward d whatever the row holds, and a chain of them visits at
// most V vertices.  sigma[x] is the number of least-cost x -> d routes
// (sigma = 1 where pcost is 0, sigma[x] = sum of sigma[n] over the next hops);
// a demand w(s, d) enters at s and is pushed down the DAG:
//   flow[x]   = demand entering at x + what the vertices upstream sent to x,
//   f(x -> n) = flow[x] * sigma[n] / sigma[x]       route split,
//   f(x -> n) = flow[x] / (number of next hops)     hop split,
//   flow[n] += f,  load[e(x -> n)] += f             e: the CSR position.
//
// Order.  There are no hop levels here: a direct link of cost 2 ties a
// two-link route of cost 1 + 1, so the next hops of one vertex sit at different
// hop counts.  Each vertex gets depth[x] = the longest next-hop chain from x:
// 0 without next hops, else 1 + max over the next hops.  It is found by pull
// sweeps: sweep k finalises every pending vertex all of whose next hops were
// final before the sweep (depth < k) -- by induction exactly the vertices of
// depth k -- and sums its sigma over them in the same walk; a vertex that
// meets a next hop that is not final stops its walk there and stays pending.
// The depth word has one writer, written once: a read that races with the
// write sees "pending" or k, and either way the reader waits for the next
// sweep; sigma[n] is read only where depth[n] < k, written before the last
// barrier.  The sweeps end when nobody is pending, after (largest depth)
// <= V - 1 of them (one more where only vertices without a next hop were
// left).  A next hop has a STRICTLY smaller depth (not necessarily depth - 1),
// which is all the push needs: it runs by descending depth, every upstream
// vertex has pushed before flow[x] is read, workgroup barriers between depths.
//
// No NaN or Inf is ever formed: a vertex whose sigma is 0 (no next hop) or
// overflowed keeps sigma 0 and sends nothing.  A vertex of finite pcost > 0
// without a next hop, sweeps that outrun V, a sigma above the double range and
// offsets outside the pair list raise the context's error word.
//
// One workgroup per row, persistent over the rows; a row without pairs is
// skipped before anything is read.  Within a depth the adds into flow[] (LDS or
// scratch) and load[] (global, shared by all workgroups) are f64 atomics, so a
// sum's last bits depend on the arrival order unless every partial sum is
// exact.  Row state: LDS (f64 sigma + f64 flow + u32 pcost + u16 depth, 22
// bytes per vertex) up to kCostEcmpLdsMaxV vertices, else a per-workgroup slice
// of the context scratch (sigma, flow and u32 depth, 20 bytes per vertex; pcost
// is read from its row).
#include "common.h"

namespace {

// The sweeps and the push are chains of dependent LDS / L2 reads per
// thread (latency, not bandwidth) and a fabric's rows are about two workgroups
// per CU: the waves that hide the latency come from the workgroup, as in
// cost_tables.hip.
constexpr int kCostEcmpThreads = 1024;
constexpr uint32_t kCostEcmpInf = SDNR_COST_INF;

template <bool LDS>
__device__ __forceinline__ double ce_ld_f64(const double *p)
{
    if (LDS) return *p;
    // scratch words are also written by atomics (performed in L2): read past L1
    return __longlong_as_double((long long)__hip_atomic_load(
        reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT));
}

template <bool LDS>
__device__ __forceinline__ void ce_st_f64(double *p, double v)
{
    if (LDS)
        *p = v;
    else
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(p),
                           (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// depth words: u16 in LDS (a depth is < V <= kCostEcmpLdsMaxV), u32 in scratch,
// where other waves of the workgroup write them: agent-scope accesses;
// kPending (above every sweep number) marks a vertex that is not final yet
template <bool LDS>
struct Depth;
template <>
struct Depth<true> {
    typedef uint16_t T;
    static constexpr int kPending = 0xFFFF;
    static __device__ __forceinline__ int ld(const T *p) { return (int)*p; }
    static __device__ __forceinline__ void st(T *p, int v) { *p = (T)v; }
};
template <>
struct Depth<false> {
    typedef uint32_t T;
    static constexpr int kPending = 0x7FFFFFFF;
    static __device__ __forceinline__ int ld(const T *p)
    {
        return (int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void st(T *p, int v)
    {
        __hip_atomic_store(p, (T)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// hop: sigma[x] holds the number of next hops instead of the route count
template <bool LDS>
__global__ __launch_bounds__(kCostEcmpThreads) void cost_ecmp_loads_kernel(
    int V, int nrows, int hop, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const uint32_t *__restrict__ cost,
    const uint32_t *__restrict__ pcost, const int64_t *__restrict__ pair_off, int64_t pair_lo,
    int64_t pair_hi, const int32_t *__restrict__ srcs, const uint64_t *__restrict__ weight,
    double *__restrict__ load, unsigned char *__restrict__ scratch, size_t scratch_stride,
    int *__restrict__ err)
{
    typedef Depth<LDS> Dp;
    typedef typename Dp::T depth_t;
    // dynamic LDS, LDS form: sigma f64 [V] | flow f64 [V] | pcost u32 [V] | depth u16 [V]
    extern __shared__ __attribute__((aligned(16))) unsigned char cost_ecmp_lds[];
    unsigned char *base = LDS ? cost_ecmp_lds : scratch + (size_t)blockIdx.x * scratch_stride;
    double *sigma = reinterpret_cast<double *>(base);
    double *flow = sigma + V;
    // LDS: flow | pcost | depth; scratch: flow | depth
    uint32_t *pc_lds = reinterpret_cast<uint32_t *>(flow + V);
    depth_t *depth = LDS ? reinterpret_cast<depth_t *>(pc_lds + V)
                         : reinterpret_cast<depth_t *>(flow + V);
    const int tid = (int)threadIdx.x;

    for (int r = (int)blockIdx.x; r < nrows; r += (int)gridDim.x) {
        const int64_t lo = pair_off[r], hi = pair_off[r + 1];
        if (lo < pair_lo || hi > pair_hi || hi < lo) {     // offsets outside the pair list
            if (tid == 0) atomicOr(err, kErrCostEcmpLoads);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no demand)
        const uint32_t *prow = pcost + (size_t)r * (size_t)V;
        const uint32_t *pc = LDS ? pc_lds : prow;

        // 1. flow = 0; the destination (pcost 0) and the unreachable are final at depth 0
        for (int x = tid; x < V; x += kCostEcmpThreads) {
            const uint32_t px = prow[x];
            if (LDS) pc_lds[x] = px;
            ce_st_f64<LDS>(&sigma[x], (px == 0 && !hop) ? 1.0 : 0.0);
            ce_st_f64<LDS>(&flow[x], 0.0);
            Dp::st(&depth[x], (px == 0 || px == kCostEcmpInf) ? 0 : Dp::kPending);
        }
        __syncthreads();

        // 2. depth and sigma: sweep k finalises the vertices whose longest chain is k
        //    (hop split: sigma = the number of next hops)
        bool done = false;
        int top = 0;
        for (int k = 1; k <= V; ++k) {
            int pending = 0;
            for (int x = tid; x < V; x += kCostEcmpThreads) {
                if (Dp::ld(&depth[x]) != Dp::kPending) continue;
                const uint32_t px = pc[x];
                double c = 0.0;
                bool any = false, ready = true;
                const int re = row_ptr[x + 1];
                for (int e = row_ptr[x]; e < re; ++e) {
                    const int n = col[e];
                    const uint32_t pn = pc[n];
                    // (64-bit sum: a row that is no labelling must not wrap into a tie)
                    if (pn == kCostEcmpInf || (uint64_t)pn + cost[e] != (uint64_t)px) continue;
                    if (Dp::ld(&depth[n]) >= k) {          // pending, or finalised in this sweep
                        ready = false;
                        break;
                    }
                    any = true;
                    c += hop ? 1.0 : ce_ld_f64<LDS>(&sigma[n]);
                }
                if (!ready) {
                    pending = 1;
                    continue;
                }
                // no next hop (a finite pcost > 0 that no link explains), dead next hops, overflow
                if (!(c > 0.0) || c > 1.7976931348623157e308) {
                    atomicOr(err, kErrCostEcmpLoads);
                    c = 0.0;
                }
                ce_st_f64<LDS>(&sigma[x], c);
                Dp::st(&depth[x], any ? k : 0);
            }
            top = k;
            if (!__syncthreads_or(pending)) {
                done = true;
                break;
            }
        }
        if (!done) {                                       // (uniform) no DAG of V vertices does that
            if (tid == 0) atomicOr(err, kErrCostEcmpLoads);
            continue;
        }

        // 3. the row's demand enters at its sources
        for (int64_t i = lo + tid; i < hi; i += kCostEcmpThreads) {
            const int s = srcs[i];
            if (s < 0 || s >= V) continue;
            const uint32_t ps = pc[s];
            if (ps == 0 || ps == kCostEcmpInf) continue;   // s == d, unreachable
            const uint64_t w = weight ? weight[i] : 1ull;
            if (w) atomicAdd(&flow[s], (double)w);
        }
        __syncthreads();

        // 4. push, deepest first
        for (int D = top; D >= 1; --D) {
            for (int x = tid; x < V; x += kCostEcmpThreads) {
                if (Dp::ld(&depth[x]) != D) continue;
                const double f = ce_ld_f64<LDS>(&flow[x]);
                const double sx = ce_ld_f64<LDS>(&sigma[x]);
                if (!(f > 0.0) || !(sx > 0.0)) continue;   // (sx == 0: reported in step 2)
                const uint32_t px = pc[x];
                const int re = row_ptr[x + 1];
                for (int e = row_ptr[x]; e < re; ++e) {
                    const int n = col[e];
                    const uint32_t pn = pc[n];
                    if (pn == kCostEcmpInf || (uint64_t)pn + cost[e] != (uint64_t)px) continue;
                    // sigma[n] <= sigma[x]: the share is in [0, 1]
                    const double g = hop ? f / sx : f * (ce_ld_f64<LDS>(&sigma[n]) / sx);
                    if (!(g > 0.0)) continue;
                    if (pn != 0) atomicAdd(&flow[n], g);   // (pcost 0: the destination absorbs)
                    atomicAdd(&load[e], g);
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace

int sdnr_launch_cost_ecmp_link_loads(sdnr_ctx *ctx, const uint32_t *d_pcost, int32_t nrows,
                                     const int64_t *d_pair_off, int64_t pair_lo, int64_t pair_hi,
                                     const int32_t *d_srcs, const uint64_t *d_weight,
                                     double *d_load, bool hop)
{
    const int V = ctx->V;
    ctx->last_launches = 1;
    if (V <= kCostEcmpLdsMaxV) {
        const size_t lds = ((size_t)V * kCostEcmpBytesPerV + 15) & ~(size_t)15;
        auto fn = cost_ecmp_loads_kernel<true>;
        sdnr_allow_lds(reinterpret_cast<const void *>(fn), lds);
        int per_cu = (int)(SDNR_LDS_PER_CU / (lds ? lds : 1));
        per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);     // 2048 threads per CU
        int64_t g = (int64_t)ctx->num_cus * per_cu;
        if (g > nrows) g = nrows;
        ctx->last_kernel = "cost_ecmp_loads_kernel<lds>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kCostEcmpThreads), lds, ctx->stream, V,
                           nrows, hop ? 1 : 0, ctx->row_ptr, ctx->col, ctx->cost, d_pcost,
                           d_pair_off, pair_lo, pair_hi, d_srcs, d_weight, d_load,
                           (unsigned char *)nullptr, (size_t)0, ctx->d_err);
    } else {
        // per workgroup: sigma, flow and u32 depths, 256-byte aligned
        const size_t stride = (((size_t)V * 20) + 255) & ~(size_t)255;
        int64_t g = (int64_t)ctx->num_cus * 2;
        if (g > nrows) g = nrows;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
        const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, stride * (size_t)g);
        if (rc) return rc;
        ctx->last_kernel = "cost_ecmp_loads_kernel<global>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(cost_ecmp_loads_kernel<false>, dim3((unsigned)g),
                           dim3(kCostEcmpThreads), 0, ctx->stream, V, nrows, hop ? 1 : 0,
                           ctx->row_ptr, ctx->col, ctx->cost, d_pcost, d_pair_off, pair_lo,
                           pair_hi, d_srcs, d_weight, d_load,
                           static_cast<unsigned char *>(ctx->scratch), stride, ctx->d_err);
    }
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}
