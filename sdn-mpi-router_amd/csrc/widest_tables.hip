// widest_tables.hip -- least-loaded routes: min-max link utilisation within
// the least-cost (ECMP) set.
//
// sdnr_cost_tables names, per destination d, ONE least-cost route per switch:
// the lexicographically smallest.  The least-cost routes toward d form a DAG:
// link e = (x -> n) is TIGHT when pcost[n] != INF and pcost[n] + cost[e] ==
// pcost[x].  Given a utilisation util[e] per link (what the port counters
// measured, or what a job admitted so far adds to it), this kernel picks inside
// that DAG the route whose busiest link is the least busy:
//   bott[x] = min over tight e = (x -> n) of max(util[e], bott[n]),
//   bott[d] = 0, bott[x] = 0xFFFFFFFF where pcost[x] is INF,
//   nh[x]   = the tight link of the smallest key
//             (max(util[e], bott[n]), util[e], n), compared lexicographically:
//             the best bottleneck, then the emptier first link (the flow's own
//             switch sees that one directly), then the smaller neighbour
//             (sdnr_cost_tables' rule, so equal utilisation changes nothing).
// Consequences:
//   * following nh from x gives a least-cost route whose busiest link carries
//     exactly bott[x] (the key's first component is bott[x], and the next hop's
//     own choice attains bott[n]);
//   * an nh row is an in-tree toward d (a tight link lowers pcost strictly), so
//     sdnr_link_loads with SDNR_LOADS_TO_ROOT takes it as it is;
//   * with util all zero, or all equal, every tight link has the same first two
//     key components and nh / nh_port are sdnr_cost_tables' bit for bit;
//   * a link that is not tight is never used, however empty it is.
// Everything is integer and bit-exact.
//
// Costs are >= 1, so the tight links lower pcost strictly: the recurrence runs
// over a DAG and has one solution.  It is solved as cost_tables.hip solves its
// own: pull sweeps in place.  The bott word of vertex x has one writer, the
// thread that owns x; it starts at INF (0 at d) and only decreases, and every
// value it takes is max(util[e], bott[n]) for a value bott[n] that was stored
// before -- by induction the busiest link of a real tight route x -> d.  A read
// that races with a store sees the old or the new word, INF or the bottleneck
// of a real route, both upper bounds of the solution: no atomics, no second
// generation.  util is at most 0xFFFFFFFE, so max(util[e], bott[n]) is INF
// exactly when bott[n] still is.  After sweep k every vertex whose longest
// tight route has <= k links is final, so DAG depth + 1 sweeps reach the fixed
// point, the last one idle (__syncthreads_or(changed)); V sweeps always
// suffice, and a run that needs more raises the context's error word.  So does
// a row that is no least-cost labelling: pcost[d] != 0, or a vertex of finite
// cost > 0 whose bott is still INF at the fixed point (it, or a vertex below
// it, has no tight link).  The other rows of the call are unaffected.
//
// One workgroup takes a batch of B destinations at once, persistent over the
// batches.  A sweep needs pcost AND bott of the vertex and of each neighbour,
// so a vertex's record is 2 B words, pcost[0..B) | bott[0..B), read as B / 2
// 16-byte quads: twice cost_tables.hip's words per relaxation and destination.
// Four forms, chosen from V alone: records in LDS with B = 6 up to
// kWidestLdsMaxV6 vertices (48 bytes per vertex), B = 4 up to kWidestLdsMaxV4
// (32 bytes), B = 2 up to kWidestLdsMaxV (16 bytes), else B = 4 in a
// per-workgroup slice of the context scratch, read and written with
// agent-scope relaxed accesses.
// The last pass of the same kernel stores bott and scans for the next hop.
#include "common.h"

namespace {

constexpr int kWidestThreads = 1024;               // as cost_tables.hip: the waves hide the LDS chain
constexpr uint32_t kWidestInf = SDNR_COST_INF;
constexpr uint32_t kWidestUtilMax = 0xFFFFFFFEu;

// a vertex's record: pc[j] = pcost, b[j] = bott of the batch's j-th destination
template <int B>
struct WidestRec {
    static_assert(B == 2 || B == 4 || B == 6, "a record is whole 16-byte quads");
    uint32_t pc[B], b[B];
};

template <bool LDS, int B>
__device__ __forceinline__ WidestRec<B> ld_rec(const uint32_t *recs, int x)
{
    WidestRec<B> r;
    const uint32_t *p = recs + (size_t)x * (2 * B);
    if (LDS) {
        uint32_t w[2 * B];
#pragma unroll
        for (int q = 0; q < B / 2; ++q) {
            const uint4 t = reinterpret_cast<const uint4 *>(p)[q];
            w[4 * q] = t.x;
            w[4 * q + 1] = t.y;
            w[4 * q + 2] = t.z;
            w[4 * q + 3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < B; ++j) {
            r.pc[j] = w[j];
            r.b[j] = w[B + j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < B; ++j) {
            r.pc[j] = __hip_atomic_load(p + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r.b[j] = __hip_atomic_load(p + B + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    return r;
}

// the bott half of a record (the pcost half is written once, by st_rec); it
// starts 4 B bytes into the record: 8-byte aligned for every B
template <bool LDS, int B>
__device__ __forceinline__ void st_bott(uint32_t *recs, int x, const uint32_t (&b)[B])
{
    uint32_t *p = recs + (size_t)x * (2 * B) + B;
    if (LDS) {
#pragma unroll
        for (int q = 0; q < B / 2; ++q)
            reinterpret_cast<uint2 *>(p)[q] = make_uint2(b[2 * q], b[2 * q + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < B; ++j)
            __hip_atomic_store(p + j, b[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool LDS, int B>
__device__ __forceinline__ void st_rec(uint32_t *recs, int x, const WidestRec<B> &r)
{
    uint32_t *p = recs + (size_t)x * (2 * B);
    if (LDS) {
#pragma unroll
        for (int j = 0; j < B; ++j) p[j] = r.pc[j];
    } else {
#pragma unroll
        for (int j = 0; j < B; ++j)
            __hip_atomic_store(p + j, r.pc[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    st_bott<LDS, B>(recs, x, r.b);
}

// e = (x -> n) is tight for a vertex of finite cost ps: pn finite and pn + c ==
// ps.  c >= 1 and ps != INF make pn < ps imply pn != INF; no sum can wrap.
// (bitwise, not short-circuit: the sweep's loop body stays free of branches, so
// its unrolled copies issue their col / LDS reads together)
__device__ __forceinline__ bool widest_tight(uint32_t ps, uint32_t pn, uint32_t c)
{
    return (ps != kWidestInf) & (pn < ps) & (ps - pn == c);
}

// COST: per-link costs uploaded (else every link costs 1)
template <bool LDS, int B, bool COST>
__global__ __launch_bounds__(kWidestThreads) void widest_tables_kernel(
    int V, int ndst, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ port, const uint32_t *__restrict__ cost,
    const uint32_t *__restrict__ util, const uint32_t *__restrict__ pcost,
    const int32_t *__restrict__ dst, uint32_t *__restrict__ bott, int32_t *__restrict__ nh,
    int32_t *__restrict__ nh_port, uint32_t *__restrict__ scratch, size_t scratch_stride,
    int *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t widest_lds[];
    uint32_t *recs = LDS ? widest_lds : scratch + (size_t)blockIdx.x * scratch_stride;
    using Rec = WidestRec<B>;
    const int tid = (int)threadIdx.x;
    const int nbatch = (ndst + B - 1) / B;

    for (int bt = (int)blockIdx.x; bt < nbatch; bt += (int)gridDim.x) {
        // the batch's destinations (-1: past the end / no vertex: an empty row)
        int d[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const int i = bt * B + j;
            const int dj = i < ndst ? dst[i] : -1;
            d[j] = (dj < 0 || dj >= V) ? -1 : dj;
        }

        // 1. the caller's pcost rows beside bott[d] = 0, INF elsewhere
        int bad = 0;
        for (int x = tid; x < V; x += kWidestThreads) {
            Rec r;
#pragma unroll
            for (int j = 0; j < B; ++j) {
                r.pc[j] = d[j] < 0 ? kWidestInf
                                   : pcost[(size_t)(bt * B + j) * (size_t)V + (size_t)x];
                r.b[j] = x == d[j] ? 0u : kWidestInf;
                if (x == d[j] && r.pc[j] != 0) bad = 1;    // no least-cost row of d
            }
            st_rec<LDS, B>(recs, x, r);
        }
        if (bad) atomicOr(err, kErrWidest);
        __syncthreads();

        // 2. sweeps until one changes nothing
        bool done = false;
        for (int sweep = 0; sweep < V; ++sweep) {
            int changed = 0;
            for (int x = tid; x < V; x += kWidestThreads) {
                const Rec cur = ld_rec<LDS, B>(recs, x);
                uint32_t best[B];
#pragma unroll
                for (int j = 0; j < B; ++j) best[j] = cur.b[j];
                const int re = row_ptr[x + 1];
#pragma unroll 4
                for (int e = row_ptr[x]; e < re; ++e) {
                    const Rec nv = ld_rec<LDS, B>(recs, col[e]);
                    const uint32_t c = COST ? cost[e] : 1u;
                    const uint32_t u = min(util[e], kWidestUtilMax);
#pragma unroll
                    for (int j = 0; j < B; ++j) {
                        const uint32_t m = max(u, nv.b[j]);     // INF while bott[n] is
                        best[j] = min(best[j],
                                      widest_tight(cur.pc[j], nv.pc[j], c) ? m : kWidestInf);
                    }
                }
                bool lower = false;
#pragma unroll
                for (int j = 0; j < B; ++j) lower |= best[j] != cur.b[j];
                if (lower) {
                    st_bott<LDS, B>(recs, x, best);
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) {
                done = true;
                break;
            }
        }
        if (!done && tid == 0) atomicOr(err, kErrWidest);

        // 3. tables: bott, and the tight link of the smallest (max, util, n)
        bad = 0;
        for (int x = tid; x < V; x += kWidestThreads) {
            const Rec cur = ld_rec<LDS, B>(recs, x);
            int at[B];
            uint64_t key[B];                               // max << 32 | util; rows ascend in n
#pragma unroll
            for (int j = 0; j < B; ++j) {
                at[j] = -1;
                key[j] = ~(uint64_t)0;
                // finite cost > 0 and no route inside the DAG: no labelling of this graph
                if (cur.pc[j] != kWidestInf && cur.pc[j] != 0 && cur.b[j] == kWidestInf) bad = 1;
            }
            if (nh) {
                const int re = row_ptr[x + 1];
#pragma unroll 4
                for (int e = row_ptr[x]; e < re; ++e) {
                    const Rec nv = ld_rec<LDS, B>(recs, col[e]);
                    const uint32_t c = COST ? cost[e] : 1u;
                    const uint32_t u = min(util[e], kWidestUtilMax);
#pragma unroll
                    for (int j = 0; j < B; ++j) {
                        const uint64_t k = (uint64_t)max(u, nv.b[j]) << 32 | u;
                        const bool take = widest_tight(cur.pc[j], nv.pc[j], c) &
                                          (nv.b[j] != kWidestInf) & (k < key[j]);
                        key[j] = take ? k : key[j];
                        at[j] = take ? e : at[j];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const int i = bt * B + j;
                if (i >= ndst) continue;
                const size_t o = (size_t)i * (size_t)V + (size_t)x;
                bott[o] = cur.b[j];
                if (nh) {
                    // (x == d: pcost 0, nothing below it; pcost INF: nothing tight)
                    nh[o] = at[j] < 0 ? -1 : col[at[j]];
                    nh_port[o] = at[j] < 0 ? -1 : port[at[j]];
                }
            }
        }
        if (bad) atomicOr(err, kErrWidest);
        __syncthreads();                                   // the records are reused by the next batch
    }
}

template <int B, bool COST>
int launch_lds(sdnr_ctx *ctx, const char *name, const uint32_t *cost, const uint32_t *d_pcost,
               const uint32_t *d_util, const int32_t *d_dst, int32_t ndst, uint32_t *d_bott,
               int32_t *d_nh, int32_t *d_nh_port)
{
    const int V = ctx->V;
    const int64_t nbatch = ((int64_t)ndst + B - 1) / B;
    const size_t lds = (size_t)V * 2 * B * sizeof(uint32_t);
    auto fn = widest_tables_kernel<true, B, COST>;
    sdnr_allow_lds(reinterpret_cast<const void *>(fn), lds);
    int per_cu = (int)(SDNR_LDS_PER_CU / (lds ? lds : 1));
    per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);         // 2048 threads per CU
    int64_t g = (int64_t)ctx->num_cus * per_cu;
    if (g > nbatch) g = nbatch;
    ctx->last_kernel = name;
    ctx->last_grid = g;
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kWidestThreads), lds, ctx->stream, V, ndst,
                       ctx->row_ptr, ctx->col, ctx->port, cost, d_util, d_pcost, d_dst, d_bott,
                       d_nh, d_nh_port, (uint32_t *)nullptr, (size_t)0, ctx->d_err);
    return SDNR_OK;
}

}  // namespace

int sdnr_launch_widest_tables(sdnr_ctx *ctx, const uint32_t *d_pcost, const uint32_t *d_util,
                              const int32_t *d_dst, int32_t ndst, uint32_t *d_bott, int32_t *d_nh,
                              int32_t *d_nh_port)
{
    const int V = ctx->V;
    const uint32_t *cost = ctx->has_cost ? ctx->cost : nullptr;    // none: every link costs 1
    int rc;
    ctx->last_launches = 1;
    if (V <= kWidestLdsMaxV6) {
        const char *name = "widest_tables_kernel<lds,6>";
        rc = cost ? launch_lds<6, true>(ctx, name, cost, d_pcost, d_util, d_dst, ndst, d_bott,
                                        d_nh, d_nh_port)
                  : launch_lds<6, false>(ctx, name, cost, d_pcost, d_util, d_dst, ndst, d_bott,
                                         d_nh, d_nh_port);
        if (rc) return rc;
    } else if (V <= kWidestLdsMaxV4) {
        const char *name = "widest_tables_kernel<lds,4>";
        rc = cost ? launch_lds<4, true>(ctx, name, cost, d_pcost, d_util, d_dst, ndst, d_bott,
                                        d_nh, d_nh_port)
                  : launch_lds<4, false>(ctx, name, cost, d_pcost, d_util, d_dst, ndst, d_bott,
                                         d_nh, d_nh_port);
        if (rc) return rc;
    } else if (V <= kWidestLdsMaxV) {
        const char *name = "widest_tables_kernel<lds,2>";
        rc = cost ? launch_lds<2, true>(ctx, name, cost, d_pcost, d_util, d_dst, ndst, d_bott,
                                        d_nh, d_nh_port)
                  : launch_lds<2, false>(ctx, name, cost, d_pcost, d_util, d_dst, ndst, d_bott,
                                         d_nh, d_nh_port);
        if (rc) return rc;
    } else {
        // per workgroup: one [V][8] u32 slice, 256-byte aligned
        constexpr int B = 4;
        const int64_t nbatch = ((int64_t)ndst + B - 1) / B;
        const size_t stride = (((size_t)V * 2 * B * sizeof(uint32_t)) + 255) & ~(size_t)255;
        int64_t g = (int64_t)ctx->num_cus * 2;
        if (g > nbatch) g = nbatch;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
        if ((rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, stride * (size_t)g))) return rc;
        ctx->last_kernel = "widest_tables_kernel<global,4>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        auto fn = cost ? widest_tables_kernel<false, B, true> : widest_tables_kernel<false, B, false>;
        hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kWidestThreads), 0, ctx->stream, V, ndst,
                           ctx->row_ptr, ctx->col, ctx->port, cost, d_util, d_pcost, d_dst, d_bott,
                           d_nh, d_nh_port, static_cast<uint32_t *>(ctx->scratch),
                           stride / sizeof(uint32_t), ctx->d_err);
    }
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}
