// ecmp_loads.hip -- per-link loads of a traffic matrix split over EVERY
// shortest route (ECMP), where loads.hip puts a pair on one route.
//
// For a destination row d, dist[x] is the hop count from x to d; the next hops
// of a vertex x of level L = dist[x] > 0 are its out-neighbours of level L - 1
// and sigma[x] is the number of shortest x -> d routes (sigma[d] = 1,
// sigma[x] = sum of sigma[n] over the next hops n).  A demand w(s, d) enters at
// s and is pushed level by level toward d (Brandes-style dependency
// accumulation, O(E) per row whatever the number of pairs or routes):
//   flow[x]   = demand entering at x + what the level above sent to x,
//   f(x -> n) = flow[x] * sigma[n] / sigma[x]       route split: every one of
//               the pair's sigma[s] routes carries w / sigma[s],
//   f(x -> n) = flow[x] / (number of next hops)     hop split (an OpenFlow
//               select group per switch),
//   flow[n] += f,  load[e(x -> n)] += f             e: the CSR position.
// sigma is a double: it does not saturate where the u64 counts of ecmp.hip do
// (2^70 routes are exact; above 1.8e308 the row is reported).  Every term is
// non-negative, so no cancellation; no NaN or Inf is ever formed: a vertex
// whose sigma is 0 (no next hop) or overflowed keeps sigma 0, sends nothing and
// raises the context's error word.
//
// One workgroup per row, persistent over the rows; a row without pairs is
// skipped before anything is read.  Levels are separated by workgroup
// barriers; within a level the adds into flow[] (LDS or scratch) and load[]
// (global, shared by all workgroups) are f64 atomics, so a sum's last bits
// depend on the arrival order unless every partial sum is exact.  Row state:
// LDS (u16 levels + f64 sigma + f64 flow, 18 bytes per vertex) up to
// kEcmpLoadsLdsMaxV vertices, else a per-workgroup slice of the context scratch
// (sigma and flow; the levels are read from the dist row).
#include "common.h"

namespace {

constexpr int kEcmpLoadsThreads = 512;

template <bool LDS>
__device__ __forceinline__ double ld_f64(const double *p)
{
    if (LDS) return *p;
    // scratch words are also written by atomics (performed in L2): read past L1
    return __longlong_as_double((long long)__hip_atomic_load(
        reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT));
}

// hop: sigma[x] holds the number of next hops instead of the route count
template <bool LDS>
__global__ __launch_bounds__(kEcmpLoadsThreads) void ecmp_loads_kernel(
    int V, int nrows, int hop, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const uint16_t *__restrict__ dist,
    const int64_t *__restrict__ pair_off, int64_t pair_lo, int64_t pair_hi,
    const int32_t *__restrict__ srcs, const uint64_t *__restrict__ weight,
    double *__restrict__ load, unsigned char *__restrict__ scratch, size_t scratch_stride,
    int *__restrict__ err)
{
    // dynamic LDS: ctl (16 bytes) | LDS form: sigma f64 [V] | flow f64 [V] | levels u16 [V]
    extern __shared__ __attribute__((aligned(16))) unsigned char ecmp_loads_lds[];
    int *ctl = reinterpret_cast<int *>(ecmp_loads_lds);
    double *sigma;
    if (LDS)
        sigma = reinterpret_cast<double *>(ecmp_loads_lds + 16);
    else
        sigma = reinterpret_cast<double *>(scratch + (size_t)blockIdx.x * scratch_stride);
    double *flow = sigma + V;
    uint16_t *lvl_lds = reinterpret_cast<uint16_t *>(ecmp_loads_lds + 16 + (size_t)V * 16);
    const int tid = (int)threadIdx.x;

    for (int r = (int)blockIdx.x; r < nrows; r += (int)gridDim.x) {
        const int64_t lo = pair_off[r], hi = pair_off[r + 1];
        if (lo < pair_lo || hi > pair_hi || hi < lo) {     // offsets outside the pair list
            if (tid == 0) atomicOr(err, kErrEcmpLoads);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no demand)
        const uint16_t *drow = dist + (size_t)r * (size_t)V;
        const uint16_t *lvl = LDS ? lvl_lds : drow;

        // 1. levels, top level; sigma[d] = 1, flow = 0
        if (tid == 0) ctl[0] = 0;
        __syncthreads();
        int mymax = 0;
        for (int x = tid; x < V; x += kEcmpLoadsThreads) {
            const uint16_t dx = drow[x];
            if (LDS) lvl_lds[x] = dx;
            sigma[x] = (dx == 0 && !hop) ? 1.0 : 0.0;
            flow[x] = 0.0;
            if (dx != 0xFFFFu && (int)dx > mymax) mymax = dx;
        }
        if (mymax) atomicMax(&ctl[0], mymax);
        __syncthreads();
        const int top = ctl[0];
        if (top >= V) {                                    // no BFS labelling has a level >= V
            if (tid == 0) atomicOr(err, kErrEcmpLoads);
            __syncthreads();                               // ctl is rewritten by the next row
            continue;
        }

        // 2. sigma by ascending level (hop split: the number of next hops)
        for (int L = 1; L <= top; ++L) {
            for (int x = tid; x < V; x += kEcmpLoadsThreads) {
                if (lvl[x] != (uint16_t)L) continue;
                double c = 0.0;
                const int re = row_ptr[x + 1];
                for (int e = row_ptr[x]; e < re; ++e) {
                    const int n = col[e];
                    if (lvl[n] == (uint16_t)(L - 1)) c += hop ? 1.0 : ld_f64<LDS>(&sigma[n]);
                }
                if (!(c > 0.0) || c > 1.7976931348623157e308) {   // no next hop / overflow
                    atomicOr(err, kErrEcmpLoads);
                    c = 0.0;
                }
                sigma[x] = c;
            }
            if (!hop) __syncthreads();                     // (hop: a vertex reads levels only)
        }
        __syncthreads();

        // 3. the row's demand enters at its sources
        for (int64_t i = lo + tid; i < hi; i += kEcmpLoadsThreads) {
            const int s = srcs[i];
            if (s < 0 || s >= V) continue;
            const uint16_t ds = lvl[s];
            if (ds == 0 || ds == 0xFFFFu) continue;        // s == d, unreachable
            const uint64_t w = weight ? weight[i] : 1ull;
            if (w) atomicAdd(&flow[s], (double)w);
        }
        __syncthreads();

        // 4. push, top level first
        for (int L = top; L >= 1; --L) {
            for (int x = tid; x < V; x += kEcmpLoadsThreads) {
                if (lvl[x] != (uint16_t)L) continue;
                const double f = ld_f64<LDS>(&flow[x]);
                const double sx = ld_f64<LDS>(&sigma[x]);
                if (!(f > 0.0) || !(sx > 0.0)) continue;   // (sx == 0: reported in step 2)
                const int re = row_ptr[x + 1];
                for (int e = row_ptr[x]; e < re; ++e) {
                    const int n = col[e];
                    if (lvl[n] != (uint16_t)(L - 1)) continue;
                    // sigma[n] <= sigma[x]: the share is in [0, 1]
                    const double g = hop ? f / sx : f * (ld_f64<LDS>(&sigma[n]) / sx);
                    if (!(g > 0.0)) continue;
                    if (L > 1) atomicAdd(&flow[n], g);
                    atomicAdd(&load[e], g);
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace

int sdnr_launch_ecmp_link_loads(sdnr_ctx *ctx, const uint16_t *d_dist, int32_t nrows,
                                const int64_t *d_pair_off, int64_t pair_lo, int64_t pair_hi,
                                const int32_t *d_srcs, const uint64_t *d_weight, double *d_load,
                                bool hop)
{
    const int V = ctx->V;
    ctx->last_launches = 1;
    if (V <= kEcmpLoadsLdsMaxV) {
        const size_t lds = (16 + (size_t)V * 18 + 15) & ~(size_t)15;
        auto fn = ecmp_loads_kernel<true>;
        sdnr_allow_lds(reinterpret_cast<const void *>(fn), lds);
        int per_cu = (int)(SDNR_LDS_PER_CU / lds);
        per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);     // 2048 threads per CU
        int64_t g = (int64_t)ctx->num_cus * per_cu;
        if (g > nrows) g = nrows;
        ctx->last_kernel = "ecmp_loads_kernel<lds>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kEcmpLoadsThreads), lds, ctx->stream, V,
                           nrows, hop ? 1 : 0, ctx->row_ptr, ctx->col, d_dist, d_pair_off, pair_lo,
                           pair_hi, d_srcs, d_weight, d_load, (unsigned char *)nullptr, (size_t)0,
                           ctx->d_err);
    } else {
        // per workgroup: sigma and flow, 256-byte aligned
        const size_t stride = (((size_t)V * 16) + 255) & ~(size_t)255;
        int64_t g = (int64_t)ctx->num_cus * 4;
        if (g > nrows) g = nrows;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
        const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, stride * (size_t)g);
        if (rc) return rc;
        ctx->last_kernel = "ecmp_loads_kernel<global>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(ecmp_loads_kernel<false>, dim3((unsigned)g), dim3(kEcmpLoadsThreads),
                           16, ctx->stream, V, nrows, hop ? 1 : 0, ctx->row_ptr, ctx->col, d_dist,
                           d_pair_off, pair_lo, pair_hi, d_srcs, d_weight, d_load,
                           static_cast<unsigned char *>(ctx->scratch), stride, ctx->d_err);
    }
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}
