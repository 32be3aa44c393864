// cost_tables.hip -- least-cost route tables under per-link costs.
//
// Where shortest.hip counts hops, every directed link e of the uploaded CSR
// carries a cost[e] >= 1 (sdnr_graph_costs: OSPF / IS-IS style metrics) and,
// for a destination d,
//   pcost[x] = min over paths x -> d of the sum of their link costs
//            = min over out-edges e = (x -> n) of cost[e] + pcost[n],
//   pcost[d] = 0, unreachable vertices hold SDNR_COST_INF,
//   nh[x]    = the smallest out-neighbour n with cost(x -> n) + pcost[n] ==
//              pcost[x] (the first such entry of x's ascending row).
// The recurrence pulls along OUT-edges, so the forward CSR is all it reads: no
// transposed graph.
//
// Pull Bellman-Ford, in place.  The word of vertex x has one writer, the
// thread that owns x, and its values only decrease, each of them the cost of a
// real path; a read that races with the write sees the old or the new value,
// both valid upper bounds, so there are no atomics and no second generation.
// A sweep ends in __syncthreads_or(changed): a sweep in which nobody wrote
// read final values only, hence the state satisfies the recurrence -- the
// fixed point.  After sweep k every vertex whose least-cost route has <= k
// links is final (costs are positive: such a route has <= V - 1 links), so V
// sweeps always suffice, the last one idle; a run that needs more raises the
// context's error word (costs the upload check would have refused).  The
// upload check (cmax * (V - 1) < 0xFFFFFFFF) keeps every sum of a finite
// value and a cost below the sentinel: plain adds, INF neighbours skipped.
//
// One workgroup relaxes a batch of B destinations at once, the rows
// interleaved as [V][B] u32: a neighbour's B costs are one or two 16-byte
// reads, and each col[e] / cost[e] fetched from L2 is relaxed into B rows.
// Workgroups are persistent over the batches.  Three forms, chosen from V
// alone: rows in LDS with B = 8 up to kCostLdsMaxV8 vertices (32 bytes per
// vertex), in LDS with B = 4 up to kCostLdsMaxV (16 bytes per vertex), else
// B = 4 in a per-workgroup slice of the context scratch, read and written with
// agent-scope relaxed accesses (the slice is written by other waves of the
// workgroup).  The last pass of the same kernel stores pcost and scans for the
// next hop; its stores run along x, one row at a time.
#include "common.h"

namespace {

// A sweep is a chain of dependent L2 -> LDS reads per thread: latency, not
// bandwidth.  All destinations of a fabric are a few hundred batches, about one
// workgroup per CU, so the waves that hide that latency have to come from the
// workgroup itself: 1,024 threads and a 4-way unrolled row loop ran the k=48
// fat-tree's 1,152 rows in 0.68 ms where 512 threads and a rolled loop took
// 1.53 ms, both with B = 4; B = 8 halves the serial CSR walks per destination
// again: 0.36 ms.
constexpr int kCostThreads = 1024;
constexpr uint32_t kCostInf = SDNR_COST_INF;

template <int B>
struct CostRow {
    static_assert(B % 4 == 0, "a batch is whole 16-byte quads");
    uint32_t v[B];
};

template <bool LDS, int B>
__device__ __forceinline__ CostRow<B> ld_cost(const uint32_t *rows, int x)
{
    CostRow<B> r;
    if (LDS) {
#pragma unroll
        for (int q = 0; q < B / 4; ++q) {
            const uint4 w = reinterpret_cast<const uint4 *>(rows + (size_t)x * B)[q];
            r.v[4 * q] = w.x;
            r.v[4 * q + 1] = w.y;
            r.v[4 * q + 2] = w.z;
            r.v[4 * q + 3] = w.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < B; ++j)
            r.v[j] = __hip_atomic_load(rows + (size_t)x * B + j, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
    }
    return r;
}

template <bool LDS, int B>
__device__ __forceinline__ void st_cost(uint32_t *rows, int x, const CostRow<B> &c)
{
    if (LDS) {
#pragma unroll
        for (int q = 0; q < B / 4; ++q)
            reinterpret_cast<uint4 *>(rows + (size_t)x * B)[q] =
                make_uint4(c.v[4 * q], c.v[4 * q + 1], c.v[4 * q + 2], c.v[4 * q + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < B; ++j)
            __hip_atomic_store(rows + (size_t)x * B + j, c.v[j], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool LDS, int B>
__global__ __launch_bounds__(kCostThreads) void cost_tables_kernel(
    int V, int ndst, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ port, const uint32_t *__restrict__ cost,
    const int32_t *__restrict__ dst, uint32_t *__restrict__ pcost, int32_t *__restrict__ nh,
    int32_t *__restrict__ nh_port, uint32_t *__restrict__ scratch, size_t scratch_stride,
    int *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t cost_lds[];
    uint32_t *rows = LDS ? cost_lds : scratch + (size_t)blockIdx.x * scratch_stride;
    using Row = CostRow<B>;
    const int tid = (int)threadIdx.x;
    const int nbatch = (ndst + B - 1) / B;

    for (int b = (int)blockIdx.x; b < nbatch; b += (int)gridDim.x) {
        // the batch's destinations (-1: past the end / no vertex: an empty row)
        int d[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const int i = b * B + j;
            const int dj = i < ndst ? dst[i] : -1;
            d[j] = (dj < 0 || dj >= V) ? -1 : dj;
        }

        // 1. pcost[d] = 0, INF elsewhere
        for (int x = tid; x < V; x += kCostThreads) {
            Row c;
#pragma unroll
            for (int j = 0; j < B; ++j) c.v[j] = x == d[j] ? 0u : kCostInf;
            st_cost<LDS, B>(rows, x, c);
        }
        __syncthreads();

        // 2. sweeps until one changes nothing
        bool done = false;
        for (int sweep = 0; sweep < V; ++sweep) {
            int changed = 0;
            for (int x = tid; x < V; x += kCostThreads) {
                const Row cur = ld_cost<LDS, B>(rows, x);
                Row best = cur;
                const int re = row_ptr[x + 1];
#pragma unroll 4
                for (int e = row_ptr[x]; e < re; ++e) {
                    const Row nv = ld_cost<LDS, B>(rows, col[e]);
                    const uint32_t c = cost[e];
#pragma unroll
                    for (int j = 0; j < B; ++j) {
                        const uint32_t t = nv.v[j] + c;      // (unused when nv is INF)
                        if (nv.v[j] != kCostInf && t < best.v[j]) best.v[j] = t;
                    }
                }
                bool lower = false;
#pragma unroll
                for (int j = 0; j < B; ++j) lower |= best.v[j] != cur.v[j];
                if (lower) {
                    st_cost<LDS, B>(rows, x, best);
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) {
                done = true;
                break;
            }
        }
        if (!done && tid == 0) atomicOr(err, kErrCostTables);

        // 3. tables: pcost, and the first least-cost entry of each row
        for (int x = tid; x < V; x += kCostThreads) {
            const Row cur = ld_cost<LDS, B>(rows, x);
            int at[B];
#pragma unroll
            for (int j = 0; j < B; ++j) at[j] = -1;
            if (nh) {
                const int re = row_ptr[x + 1];
                for (int e = row_ptr[x]; e < re; ++e) {
                    const Row nv = ld_cost<LDS, B>(rows, col[e]);
                    const uint32_t c = cost[e];
#pragma unroll
                    for (int j = 0; j < B; ++j)
                        if (at[j] < 0 && nv.v[j] != kCostInf && nv.v[j] + c == cur.v[j])
                            at[j] = e;
                }
            }
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const int i = b * B + j;
                if (i >= ndst) continue;
                const size_t o = (size_t)i * (size_t)V + (size_t)x;
                pcost[o] = cur.v[j];
                if (nh) {
                    // (cur INF: every neighbour is INF; cur 0: every sum is >= 1)
                    nh[o] = at[j] < 0 ? -1 : col[at[j]];
                    nh_port[o] = at[j] < 0 ? -1 : port[at[j]];
                }
            }
        }
        __syncthreads();                                   // the rows are reused by the next batch
    }
}

}  // namespace

template <int B>
static int launch_lds(sdnr_ctx *ctx, const char *name, const int32_t *d_dst, int32_t ndst,
                      uint32_t *d_pcost, int32_t *d_nh, int32_t *d_nh_port)
{
    const int V = ctx->V;
    const int64_t nbatch = ((int64_t)ndst + B - 1) / B;
    const size_t lds = (size_t)V * B * sizeof(uint32_t);
    auto fn = cost_tables_kernel<true, B>;
    sdnr_allow_lds(reinterpret_cast<const void *>(fn), lds);
    int per_cu = (int)(SDNR_LDS_PER_CU / (lds ? lds : 1));
    per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);         // 2048 threads per CU
    int64_t g = (int64_t)ctx->num_cus * per_cu;
    if (g > nbatch) g = nbatch;
    ctx->last_kernel = name;
    ctx->last_grid = g;
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kCostThreads), lds, ctx->stream, V, ndst,
                       ctx->row_ptr, ctx->col, ctx->port, ctx->cost, d_dst, d_pcost, d_nh,
                       d_nh_port, (uint32_t *)nullptr, (size_t)0, ctx->d_err);
    return SDNR_OK;
}

int sdnr_launch_cost_tables(sdnr_ctx *ctx, const int32_t *d_dst, int32_t ndst, uint32_t *d_pcost,
                            int32_t *d_nh, int32_t *d_nh_port)
{
    const int V = ctx->V;
    int rc;
    ctx->last_launches = 1;
    if (V <= kCostLdsMaxV8) {
        if ((rc = launch_lds<8>(ctx, "cost_tables_kernel<lds,8>", d_dst, ndst, d_pcost, d_nh,
                                d_nh_port)))
            return rc;
    } else if (V <= kCostLdsMaxV) {
        if ((rc = launch_lds<4>(ctx, "cost_tables_kernel<lds,4>", d_dst, ndst, d_pcost, d_nh,
                                d_nh_port)))
            return rc;
    } else {
        // per workgroup: one [V][4] u32 slice, 256-byte aligned
        constexpr int B = 4;
        const int64_t nbatch = ((int64_t)ndst + B - 1) / B;
        const size_t stride = (((size_t)V * B * sizeof(uint32_t)) + 255) & ~(size_t)255;
        int64_t g = (int64_t)ctx->num_cus * 2;
        if (g > nbatch) g = nbatch;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
        if ((rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, stride * (size_t)g))) return rc;
        ctx->last_kernel = "cost_tables_kernel<global,4>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL((cost_tables_kernel<false, B>), dim3((unsigned)g), dim3(kCostThreads),
                           0, ctx->stream, V, ndst, ctx->row_ptr, ctx->col, ctx->port, ctx->cost,
                           d_dst, d_pcost, d_nh, d_nh_port, static_cast<uint32_t *>(ctx->scratch),
                           stride / sizeof(uint32_t), ctx->d_err);
    }
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}
