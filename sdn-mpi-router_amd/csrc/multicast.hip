// multicast.hip -- multicast trees: the one-to-many flow entries of groups.
//
// OpenFlow 1.0 lets one flow entry carry several output actions, so a switch
// can replicate: when a root sends to a group of members along the
// controller's own routes, the links used are the set union of the members'
// routes -- one (dpid, out_port) entry per link of the union, however many
// members lie behind it (reference sdnmpi/router.py:83-104 installs the
// entries of ONE route; its one-to-many traffic floods, topology.py:150-177).
// No route is built: every member's lane walks its route through the cached
// table row and marks the links it crosses in an E-bit map of the group; the
// union is that map.
//
//   source-rooted rows (the default route: the tree of the group's root): the
//     lane climbs parent() from the member to the root.  A V-bit visited map
//     (atomic OR) makes one walk the owner of every vertex: the owner looks the
//     link parent(x) -> x up and marks it, a later walk only reads the parent.
//     Every walk still climbs to the root, read-only above its first claimed
//     vertex: the claims of several walks can close a parent cycle that none
//     of them sees on its own, and the climb's step bound is what finds it;
//   to-root rows (SDNR_MCAST_TO_ROOT: per-destination next-hop rows, one row
//     per member): the lane walks down from the root along the member's row
//     and marks every link x -> nh[x].  The rows differ, so no walk can stop
//     at another's vertex.
//
// One 256-thread workgroup per group, persistent over the groups.  The two
// maps live in LDS while their words fit kMcastLdsBytes, else in a
// per-workgroup slice of the context's scratch (global atomics).  After the
// walks the link map is counted (popcount per word, workgroup sum) and, in a
// fill call, compacted in ascending edge order: popcount per word, a
// workgroup scan over 256 words at a time, each lane writes its word's bits.
// Nothing is kept between the count call and the fill call: the fill walks
// again.  No workgroup waits on another.
#include "common.h"

namespace {

constexpr int kMcastThreads = 256;
constexpr int kMcastWaves = kMcastThreads / SDNR_WAVE;

template <bool LDS>
__device__ __forceinline__ uint32_t map_or(uint32_t *w, uint32_t bit)
{
    if (LDS) return atomicOr(w, bit);
    return __hip_atomic_fetch_or(w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ uint32_t map_word(const uint32_t *w)
{
    if (LDS) return *w;
    return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// inclusive scan of c over the workgroup (*total: the sum); two barriers
__device__ __forceinline__ int block_scan(int c, int *wave_sum, int *total)
{
    const int lane = lane_id(), wv = (int)threadIdx.x / SDNR_WAVE;
    int s = c;
    for (int d = 1; d < SDNR_WAVE; d <<= 1) {
        const int y = __shfl_up(s, d, SDNR_WAVE);
        if (lane >= d) s += y;
    }
    if (lane == SDNR_WAVE - 1) wave_sum[wv] = s;
    __syncthreads();
    int below = 0, all = 0;
    for (int k = 0; k < kMcastWaves; ++k) {
        const int ws = wave_sum[k];
        if (k < wv) below += ws;
        all += ws;
    }
    __syncthreads();                                       // wave_sum is reused
    *total = all;
    return s + below;
}

// CSR index of the tree link p -> x of a source-rooted row (-1: no such link)
__device__ __forceinline__ int tree_edge(const LoadRows &t, const int32_t *__restrict__ row_ptr,
                                         const int32_t *__restrict__ col, int p, int x, int slot)
{
    if (t.layout != SDNR_TREE_SLOT) return edge_index(row_ptr, col, p, x);
    const int e = row_ptr[p] + slot;
    return (e < row_ptr[p + 1] && col[e] == x) ? e : -1;
}

template <bool LDS>
__global__ __launch_bounds__(kMcastThreads) void multicast_trees_kernel(
    LoadRows t, int V, int E, int nrows, int ngroups, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const int32_t *__restrict__ root,
    const int64_t *__restrict__ mem_off, int64_t mem_lo, int64_t mem_hi,
    const int32_t *__restrict__ mem_row, const int32_t *__restrict__ mem_vertex,
    const uint64_t *__restrict__ weight, unsigned char *__restrict__ reached,
    long long *__restrict__ ent_cnt, const int64_t *__restrict__ ent_off, int64_t ent_lo,
    int64_t ent_hi, int32_t *__restrict__ ent_edge, unsigned long long *__restrict__ load,
    unsigned char *__restrict__ scratch, size_t scratch_stride, int *__restrict__ err)
{
    extern __shared__ uint32_t mcast_lds[];
    __shared__ int wave_sum[kMcastWaves];
    __shared__ int group_bad;
    const int vw = (V + 31) >> 5, ew = (E + 31) >> 5;
    uint32_t *vis;
    if (LDS)
        vis = mcast_lds;
    else
        vis = reinterpret_cast<uint32_t *>(scratch + (size_t)blockIdx.x * scratch_stride);
    uint32_t *lnk = vis + vw;
    const int tid = (int)threadIdx.x;

    for (int g = (int)blockIdx.x; g < ngroups; g += (int)gridDim.x) {
        const int64_t lo = mem_off[g], hi = mem_off[g + 1];
        if (lo < mem_lo || hi > mem_hi || hi < lo) {       // offsets outside the member list
            if (tid == 0) {
                atomicOr(err, kErrMcast);
                if (ent_cnt) ent_cnt[g] = 0;
            }
            continue;
        }
        if (lo == hi) {                                    // (uniform: a group without members)
            if (tid == 0 && ent_cnt) ent_cnt[g] = 0;
            continue;
        }
        const int r = root[g];
        const bool root_ok = r >= 0 && r < V;

        for (int w = tid; w < vw + ew; w += kMcastThreads) {
            if (LDS)
                vis[w] = 0;
            else
                __hip_atomic_store(&vis[w], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid == 0) group_bad = 0;
        __syncthreads();

        for (int64_t i = lo + tid; i < hi; i += kMcastThreads) {
            const int row = mem_row[i], v = mem_vertex[i];
            unsigned char ok = 0;
            bool bad = false;
            if (root_ok && row >= 0 && row < nrows && v >= 0 && v < V) {
                const size_t rb = (size_t)row * (size_t)V;
                if (v == r) {
                    ok = 1;
                } else if (t.to_root) {
                    // down from the root along the member's next-hop row
                    if ((int)t.tree[rb + r] >= 0) {
                        ok = 1;
                        int x = r, steps = 0;
                        while (x != v) {
                            const int n = (int)t.tree[rb + x];
                            if (steps++ >= V || n < 0 || n >= V) {
                                bad = true;
                                break;
                            }
                            const int e = edge_index(row_ptr, col, x, n);
                            if (e < 0 || e >= E) {
                                bad = true;
                                break;
                            }
                            map_or<LDS>(&lnk[e >> 5], 1u << (e & 31));
                            x = n;
                        }
                    }
                } else {
                    const uint32_t w = t.tree[rb + v];
                    const bool none = t.layout == SDNR_TREE_PORT16 ? (w & 0xFFFFu) == 0xFFFFu
                                                                   : w == SDNR_TREE_NONE;
                    if (!none) {
                        // up to the root; the links of the vertices this walk claims
                        ok = 1;
                        int x = v, steps = 0;
                        bool claiming = true;
                        while (x != r) {
                            int slot;
                            const int p = load_parent(t, rb, x, V, &slot, &bad);
                            if (steps++ >= V || p < 0) {
                                bad = true;
                                break;
                            }
                            if (claiming) {
                                const uint32_t bit = 1u << (x & 31);
                                if (map_or<LDS>(&vis[x >> 5], bit) & bit) {
                                    claiming = false;      // another walk owns x and all above
                                } else {
                                    const int e = tree_edge(t, row_ptr, col, p, x, slot);
                                    if (e < 0 || e >= E) {
                                        bad = true;
                                        break;
                                    }
                                    map_or<LDS>(&lnk[e >> 5], 1u << (e & 31));
                                }
                            }
                            x = p;
                        }
                    }
                }
            }
            if (bad) atomicOr(&group_bad, 1);
            if (reached) reached[i] = ok;
        }
        __syncthreads();
        if (group_bad) {                                   // (uniform) the group adds nothing
            if (tid == 0) {
                atomicOr(err, kErrMcast);
                if (ent_cnt) ent_cnt[g] = 0;
            }
            __syncthreads();                               // group_bad is reset by the next group
            continue;
        }

        // the union's size
        int mine = 0;
        for (int w = tid; w < ew; w += kMcastThreads) mine += __popc(map_word<LDS>(&lnk[w]));
        int total;
        block_scan(mine, wave_sum, &total);
        if (tid == 0 && ent_cnt) ent_cnt[g] = total;

        bool fill = ent_edge != nullptr;
        int64_t at = 0;
        if (fill) {
            at = ent_off[g];
            const int64_t end = ent_off[g + 1];
            if (at < ent_lo || end > ent_hi || end - at != (int64_t)total) {
                if (tid == 0) atomicOr(err, kErrMcast);    // not the prefix of these counts
                fill = false;
            }
        }
        const unsigned long long wt = load ? (weight ? (unsigned long long)weight[g] : 1ull) : 0ull;
        if (fill) {
            // ordered compaction, 256 words at a time
            for (int w0 = 0; w0 < ew; w0 += kMcastThreads) {
                const int w = w0 + tid;
                uint32_t bits = w < ew ? map_word<LDS>(&lnk[w]) : 0u;
                int chunk;
                const int incl = block_scan(__popc(bits), wave_sum, &chunk);
                int64_t pos = at + (incl - __popc(bits));
                while (bits) {
                    const int e = (w << 5) + (__ffs(bits) - 1);
                    bits &= bits - 1;
                    ent_edge[pos++] = e;
                    if (wt) atomicAdd(&load[e], wt);
                }
                at += chunk;
            }
        } else if (wt) {
            for (int w = tid; w < ew; w += kMcastThreads) {
                uint32_t bits = map_word<LDS>(&lnk[w]);
                while (bits) {
                    const int e = (w << 5) + (__ffs(bits) - 1);
                    bits &= bits - 1;
                    atomicAdd(&load[e], wt);
                }
            }
        }
        __syncthreads();                                   // the maps are reused by the next group
    }
}

}  // namespace

int sdnr_launch_multicast_trees(sdnr_ctx *ctx, const void *d_tree, int32_t layout, bool to_root,
                                int32_t nrows, int32_t ngroups, const int32_t *d_root,
                                const int64_t *d_mem_off, int64_t mem_lo, int64_t mem_hi,
                                const int32_t *d_mem_row, const int32_t *d_mem_vertex,
                                const uint64_t *d_weight, uint8_t *d_reached, int64_t *d_ent_cnt,
                                const int64_t *d_ent_off, int64_t ent_lo, int64_t ent_hi,
                                int32_t *d_ent_edge, uint64_t *d_load)
{
    const int V = ctx->V, E = ctx->E;
    LoadRows t{static_cast<const uint32_t *>(d_tree), layout, to_root ? 1 : 0};
    const size_t words = (size_t)((V + 31) >> 5) + (size_t)(((int64_t)E + 31) >> 5);
    unsigned long long *load = reinterpret_cast<unsigned long long *>(d_load);
    long long *cnt = reinterpret_cast<long long *>(d_ent_cnt);
    ctx->last_launches = 1;
    if (words * 4 <= kMcastLdsBytes) {
        const size_t lds = words * 4;
        auto fn = multicast_trees_kernel<true>;
        int64_t g = (int64_t)ctx->num_cus * 4;             // 4 x 32 KiB of the CU's LDS
        if (g > ngroups) g = ngroups;
        ctx->last_kernel = "multicast_trees_kernel<lds>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kMcastThreads), lds, ctx->stream, t, V, E,
                           nrows, ngroups, ctx->row_ptr, ctx->col, d_root, d_mem_off, mem_lo,
                           mem_hi, d_mem_row, d_mem_vertex, d_weight, d_reached, cnt, d_ent_off,
                           ent_lo, ent_hi, d_ent_edge, load, (unsigned char *)nullptr, (size_t)0,
                           ctx->d_err);
    } else {
        const size_t stride = (words * 4 + 255) & ~(size_t)255;
        int64_t g = (int64_t)ctx->num_cus * 4;
        if (g > ngroups) g = ngroups;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
        const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, stride * (size_t)g);
        if (rc) return rc;
        ctx->last_kernel = "multicast_trees_kernel<global>";
        ctx->last_grid = g;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL((multicast_trees_kernel<false>), dim3((unsigned)g), dim3(kMcastThreads),
                           0, ctx->stream, t, V, E, nrows, ngroups, ctx->row_ptr, ctx->col, d_root,
                           d_mem_off, mem_lo, mem_hi, d_mem_row, d_mem_vertex, d_weight, d_reached,
                           cnt, d_ent_off, ent_lo, ent_hi, d_ent_edge, load,
                           static_cast<unsigned char *>(ctx->scratch), stride, ctx->d_err);
    }
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}
