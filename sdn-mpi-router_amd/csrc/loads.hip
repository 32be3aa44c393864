// loads.hip -- per-link traffic loads of a routed traffic matrix.
//
// The controller installs one flow entry per switch of a pair's route
// (reference sdnmpi/router.py:83-104) and its monitor logs the per-port
// traffic those flows cause (sdnmpi/monitor.py).  Given the route tables and a
// demand (pairs with weights), the load of a link is the total weight of the
// pairs routed over it.  No entry is materialised: in the tree row of one
// source the load of edge parent(v) -> v is the demand destined into v's
// subtree,
//   w[v] = sum of the row's pair weights with dst == v,
//   T[v] = sum of w[x] over the subtree of v,        load[e(parent(v), v)] += T[v].
// The first-push trees are deep (94 hops on the k=48 fat-tree, 11,921 on the
// 32^3 torus), so the subtree sums use ancestor doubling, not one barrier per
// level:  A_0 = w, J_0 = parent (none for the root / unreached vertices),
//   A_{k+1}[v] = A_k[v] + sum of A_k[y] over y with J_k[y] == v,
//   J_{k+1}[y] = J_k[J_k[y]],
// until no J is valid: A_k[v] holds the demand of v's descendants less than
// 2^k levels below it, so A = T after ceil(log2(depth + 1)) rounds.  All sums
// are u64 and wrap; integer adds commute, so the result does not depend on
// the order of the atomics.
//
// One workgroup per row, persistent over the rows.  A and J are ping-pong
// buffers (a round reads generation k and writes k + 1: no vertex sees a
// half-updated neighbour): in LDS when 20 bytes per vertex fit (u64 sums, u16
// ancestors; V <= kLoadsLdsMaxV), else in a per-workgroup slice of the
// context's scratch (u32 ancestors).  The fan-in adds are LDS / global
// atomics; the edge adds at the end are global u64 atomics, one per vertex
// with a nonzero subtree sum.
//
// SDNR_LOADS_TO_ROOT runs the same rounds over per-destination next-hop rows
// (sdnr_shortest_tables' nh): the "parent" of v is nh[v], dsts[] name the
// flows' source switches and the edge is v -> nh[v], looked up in v's row.
#include "common.h"

namespace {

constexpr int kLoadsThreads = 512;

// JT: u16 (LDS, kNone 0xFFFF) or u32 (global scratch, kNone 0xFFFFFFFF)
template <typename JT, bool LDS>
__global__ __launch_bounds__(kLoadsThreads) void link_loads_kernel(
    LoadRows t, int V, int E, int nrows, int max_rounds, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const int64_t *__restrict__ pair_off, int64_t pair_lo,
    int64_t pair_hi, const int32_t *__restrict__ dsts, const uint64_t *__restrict__ weight,
    unsigned long long *__restrict__ load, unsigned char *__restrict__ scratch,
    size_t scratch_stride, int *__restrict__ err)
{
    extern __shared__ unsigned long long loads_lds[];
    constexpr JT kNone = (JT)~(JT)0;
    // generation g of the sums / ancestors: A0 + g * V, J0 + g * V
    unsigned long long *A0;
    if (LDS)
        A0 = loads_lds;
    else
        A0 = reinterpret_cast<unsigned long long *>(scratch + (size_t)blockIdx.x * scratch_stride);
    JT *J0 = reinterpret_cast<JT *>(A0 + 2 * (size_t)V);
    const int tid = (int)threadIdx.x;

    for (int r = (int)blockIdx.x; r < nrows; r += (int)gridDim.x) {
        int64_t lo = pair_off[r], hi = pair_off[r + 1];
        if (lo < pair_lo || hi > pair_hi || hi < lo) {     // offsets outside the pair list
            if (tid == 0) atomicOr(err, kErrLoadsTree);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no demand)
        const size_t rb = (size_t)r * (size_t)V;
        bool bad = false;

        // A_0 = 0, J_0 = parent
        int any0 = 0;
        for (int v = tid; v < V; v += kLoadsThreads) {
            int slot;
            const int p = load_parent(t, rb, v, V, &slot, &bad);
            A0[v] = 0;
            J0[v] = p < 0 ? kNone : (JT)p;
            any0 |= p >= 0;
        }
        int more = __syncthreads_or(any0);
        // A_0 = w
        for (int64_t i = lo + tid; i < hi; i += kLoadsThreads) {
            const int d = dsts[i];
            if (d < 0 || d >= V) continue;
            const unsigned long long w = weight ? (unsigned long long)weight[i] : 1ull;
            if (w) atomicAdd(&A0[d], w);
        }
        __syncthreads();

        int cur = 0, rounds = 0;
        while (more) {
            if (rounds == max_rounds) {                    // an ancestor chain longer than V
                bad = true;
                break;
            }
            unsigned long long *Ac = A0 + (cur ? V : 0), *An = A0 + (cur ? 0 : V);
            JT *Jc = J0 + (cur ? V : 0), *Jn = J0 + (cur ? 0 : V);
            for (int v = tid; v < V; v += kLoadsThreads)
                An[v] = LDS ? Ac[v]
                            : __hip_atomic_load(&Ac[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            int any = 0;
            for (int v = tid; v < V; v += kLoadsThreads) {
                const JT j = Jc[v];
                JT jj = kNone;
                if (j != kNone) {
                    const unsigned long long a =
                        LDS ? Ac[v]
                            : __hip_atomic_load(&Ac[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (a) atomicAdd(&An[j], a);
                    jj = Jc[j];
                    any |= jj != kNone;
                }
                Jn[v] = jj;
            }
            more = __syncthreads_or(any);
            cur ^= 1;
            ++rounds;
        }
        // (bad is per thread until here; the row is dropped by all or none)
        if (__syncthreads_or(bad ? 1 : 0)) {
            if (tid == 0) atomicOr(err, kErrLoadsTree);
            continue;
        }

        // load[e(parent(v), v)] += T[v]
        const unsigned long long *T = A0 + (cur ? V : 0);
        for (int v = tid; v < V; v += kLoadsThreads) {
            const unsigned long long x =
                LDS ? T[v] : __hip_atomic_load(&T[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!x) continue;
            int slot;
            bool b2 = false;
            const int p = load_parent(t, rb, v, V, &slot, &b2);
            if (p < 0) continue;
            int e;
            if (t.to_root) {
                e = edge_index(row_ptr, col, v, p);
            } else if (t.layout == SDNR_TREE_SLOT) {
                e = row_ptr[p] + slot;
                if (e >= row_ptr[p + 1] || col[e] != v) e = -1;
            } else {
                e = edge_index(row_ptr, col, p, v);
            }
            if (e < 0 || e >= E) {                         // a tree link the graph does not have
                atomicOr(err, kErrLoadsTree);
                continue;
            }
            atomicAdd(&load[e], x);
        }
        __syncthreads();                                   // the buffers are reused by the next row
    }
}

}  // namespace

int sdnr_launch_link_loads(sdnr_ctx *ctx, const void *d_tree, int32_t layout, bool to_root,
                           int32_t nrows, const int64_t *d_pair_off, int64_t pair_lo,
                           int64_t pair_hi, const int32_t *d_dsts, const uint64_t *d_weight,
                           uint64_t *d_load)
{
    const int V = ctx->V;
    int max_rounds = 1;                                    // ceil(log2 V) + 1
    while ((1ll << (max_rounds - 1)) < (long long)V) ++max_rounds;
    LoadRows t{static_cast<const uint32_t *>(d_tree), layout, to_root ? 1 : 0};
    unsigned long long *load = reinterpret_cast<unsigned long long *>(d_load);
    ctx->last_launches = 1;
    if (V <= kLoadsLdsMaxV) {
        const size_t lds = (size_t)V * 20;       // two u64 + two u16 generations
        auto fn = link_loads_kernel<uint16_t, true>;
        sdnr_allow_lds(reinterpret_cast<const void *>(fn), lds);
        int per_cu = (int)(SDNR_LDS_PER_CU / (lds ? lds : 1));
        per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);     // 2048 threads per CU
        int64_t g = (int64_t)ctx->num_cus * per_cu;
        if (g > nrows) g = nrows;
        ctx->last_kernel = "link_loads_kernel<lds>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kLoadsThreads), lds, ctx->stream, t, V,
                           ctx->E, nrows, max_rounds, ctx->row_ptr, ctx->col, d_pair_off, pair_lo,
                           pair_hi, d_dsts, d_weight, load, (unsigned char *)nullptr, (size_t)0,
                           ctx->d_err);
    } else {
        // per workgroup: two u64 and two u32 generations, 256-byte aligned
        const size_t stride = (((size_t)V * 24) + 255) & ~(size_t)255;
        int64_t g = ctx->num_cus;
        if (g > nrows) g = nrows;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
        const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, stride * (size_t)g);
        if (rc) return rc;
        ctx->last_kernel = "link_loads_kernel<global>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL((link_loads_kernel<uint32_t, false>), dim3((unsigned)g),
                           dim3(kLoadsThreads), 0, ctx->stream, t, V, ctx->E, nrows, max_rounds,
                           ctx->row_ptr, ctx->col, d_pair_off, pair_lo, pair_hi, d_dsts, d_weight,
                           load, static_cast<unsigned char *>(ctx->scratch), stride, ctx->d_err);
    }
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}
