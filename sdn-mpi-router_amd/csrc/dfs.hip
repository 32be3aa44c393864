// dfs.hip -- reference-exact default-route tables on gfx950.
//
// Reference: TopologyDB._find_route_dfs (sdnmpi/util/topology_db.py:59-84):
// a LIFO stack search where a switch is marked visited when it is PUSHED
// (:78-82) and neighbours are pushed in ascending dpid order (:76).  The
// parent of v is fixed by the pop that first pushes it, and stopping at the
// destination (:70-71) happens after that push, so one full traversal from
// s answers find_route(s, d) for EVERY d: the route is the path from s to d
// in the tree of first pushes.  That traversal is serial pop after pop, so
// the kernels run one source per wavefront and make the pop chain short:
//
//  * one pop = one coalesced load of u's adjacency row (ELL rows of width
//    W <= 64 are addressed as u*W: no row_ptr load on the chain), a gather of
//    the visited bits from LDS, __ballot over the row, mbcnt ranks for the
//    ascending push order, and ds_or to mark;
//  * the largest freshly pushed child is the next pop (LIFO), so it stays in
//    an SGPR instead of going through the stack;
//  * dfs_lds_kernel (V < 65536, small graphs): visited bits, stack, parent,
//    slot and depth live in LDS (10 B per vertex) and the tables are written
//    once, coalesced, after the traversal -- no global store on the chain;
//  * dfs_global_kernel (large graphs): visited bits and a 1024-entry stack
//    ring in LDS, spilled to / refilled from global scratch in halves;
//    table entries are stored as vertices are pushed.
//
// Sources are independent: persistent grid, one 64-thread workgroup per
// source, grid-stride over sources.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "common.h"

namespace {

constexpr int kRing = 1024;   // LDS stack ring entries (global mode)

template <bool ELL, bool HOPS>
__global__ __launch_bounds__(64) void dfs_lds_wide_kernel(
    int V, int W, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const int32_t *__restrict__ port,
    const int32_t *__restrict__ src, int nsrc, int32_t *__restrict__ out_parent,
    int32_t *__restrict__ out_port, int32_t *__restrict__ out_hops)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int VW = (V + 31) >> 5;
    const int VWp = (VW + 3) & ~3;
    uint32_t *vis = lds;                       // visited bits
    uint32_t *stk = vis + VWp;                 // stack: v | depth << 16
    uint32_t *ps = stk + V;                    // parent | row slot << 16
    uint16_t *dep = reinterpret_cast<uint16_t *>(ps + V);
    const int lane = lane_id();

    for (int si = blockIdx.x; si < nsrc; si += gridDim.x) {
        const int s = uniform(src[si]);
        int32_t *prow = out_parent + (size_t)si * V;
        int32_t *trow = out_port + (size_t)si * V;
        int32_t *hrow = HOPS ? out_hops + (size_t)si * V : nullptr;
        if (s < 0 || s >= V) {                 // unknown source: empty row
            for (int v = lane; v < V; v += SDNR_WAVE) {
                prow[v] = -1;
                trow[v] = -1;
                if (HOPS) hrow[v] = -1;
            }
            continue;
        }
        for (int w = lane; w < VW; w += SDNR_WAVE) vis[w] = 0u;
        __syncthreads();
        if (lane == 0) {
            vis[s >> 5] = 1u << (s & 31);
            ps[s] = (uint32_t)s;
            dep[s] = 0;
        }
        __syncthreads();

        int sp = 0, u = s, du = 0;
        for (;;) {
            int rs, re;
            if (ELL) {
                rs = u * W;
                re = rs + W;
            } else {
                rs = row_ptr[u];
                re = row_ptr[u + 1];
            }
            int nxt = -1;
            for (int base = rs; base < re; base += SDNR_WAVE) {
                const int e = base + lane;
                int v = -1;
                if (e < re) v = col[e];
                bool unv = false;
                if (v >= 0) unv = ((vis[v >> 5] >> (v & 31)) & 1u) == 0u;
                const uint64_t m = __ballot(unv);
                if (m == 0) continue;
                const int cnt = __popcll(m);
                const int rank = lanes_below(m);
                const uint32_t dtag = (uint32_t)(du + 1) << 16;
                if (nxt >= 0) {                // previous chunk's top goes below
                    if (lane == 0) stk[sp] = (uint32_t)nxt | dtag;
                    sp += 1;
                }
                if (unv) {
                    atomicOr(&vis[v >> 5], 1u << (v & 31));
                    ps[v] = (uint32_t)u | ((uint32_t)(e - rs) << 16);
                    if (HOPS) dep[v] = (uint16_t)(du + 1);
                    if (rank < cnt - 1) stk[sp + rank] = (uint32_t)v | dtag;
                }
                sp += cnt - 1;
                nxt = read_lane(v, highest_lane(m));
            }
            if (nxt >= 0) {
                u = nxt;
                du += 1;
            } else {
                if (sp == 0) break;
                sp -= 1;
                const uint32_t ent = (uint32_t)uniform((int)stk[sp]);
                u = (int)(ent & 0xFFFFu);
                du = (int)(ent >> 16);
            }
        }
        __syncthreads();

        for (int v = lane; v < V; v += SDNR_WAVE) {
            int p = -1, pt = -1, h = -1;
            if ((vis[v >> 5] >> (v & 31)) & 1u) {
                const uint32_t x = ps[v];
                p = (int)(x & 0xFFFFu);
                if (v == s) {
                    h = 0;
                } else {
                    const int slot = (int)(x >> 16);
                    pt = ELL ? port[(size_t)p * W + slot] : port[row_ptr[p] + slot];
                    h = HOPS ? (int)dep[v] : 0;
                }
            }
            prow[v] = p;
            trow[v] = pt;
            if (HOPS) hrow[v] = h;
        }
        __syncthreads();
    }
}

template <bool ELL, bool HOPS>
__global__ __launch_bounds__(64) void dfs_global_wide_kernel(
    int V, int W, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const int32_t *__restrict__ port,
    const int32_t *__restrict__ src, int nsrc, int32_t *__restrict__ out_parent,
    int32_t *__restrict__ out_port, int32_t *__restrict__ out_hops,
    uint2 *__restrict__ spill_all)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int VW = (V + 31) >> 5;
    const int VWp = (VW + 3) & ~3;
    uint32_t *vis = lds;
    uint2 *ring = reinterpret_cast<uint2 *>(vis + VWp);   // (v, depth)
    uint2 *spill = spill_all + (size_t)blockIdx.x * (size_t)V;
    const int lane = lane_id();

    for (int si = blockIdx.x; si < nsrc; si += gridDim.x) {
        const int s = uniform(src[si]);
        int32_t *prow = out_parent + (size_t)si * V;
        int32_t *trow = out_port + (size_t)si * V;
        int32_t *hrow = HOPS ? out_hops + (size_t)si * V : nullptr;
        if (s < 0 || s >= V) {
            for (int v = lane; v < V; v += SDNR_WAVE) {
                prow[v] = -1;
                trow[v] = -1;
                if (HOPS) hrow[v] = -1;
            }
            continue;
        }
        for (int w = lane; w < VW; w += SDNR_WAVE) vis[w] = 0u;
        __syncthreads();
        if (lane == 0) {
            vis[s >> 5] = 1u << (s & 31);
            prow[s] = s;
            trow[s] = -1;
            if (HOPS) hrow[s] = 0;
        }
        __syncthreads();

        int lsp = 0, bot = 0, gsp = 0;        // ring depth, ring bottom, spilled
        int u = s, du = 0;
        for (;;) {
            int rs, re;
            if (ELL) {
                rs = u * W;
                re = rs + W;
            } else {
                rs = row_ptr[u];
                re = row_ptr[u + 1];
            }
            int nxt = -1;
            for (int base = rs; base < re; base += SDNR_WAVE) {
                const int e = base + lane;
                int v = -1, pt = -1;
                if (e < re) {
                    v = col[e];
                    pt = port[e];
                }
                bool unv = false;
                if (v >= 0) unv = ((vis[v >> 5] >> (v & 31)) & 1u) == 0u;
                const uint64_t m = __ballot(unv);
                if (m == 0) continue;
                const int cnt = __popcll(m);
                const int rank = lanes_below(m);
                if (unv) {
                    atomicOr(&vis[v >> 5], 1u << (v & 31));
                    prow[v] = u;
                    trow[v] = pt;
                    if (HOPS) hrow[v] = du + 1;
                }
                if (lsp + cnt > kRing) {       // spill the oldest half
                    for (int i = lane; i < kRing / 2; i += SDNR_WAVE)
                        spill[gsp + i] = ring[(bot + i) & (kRing - 1)];
                    gsp += kRing / 2;
                    bot = (bot + kRing / 2) & (kRing - 1);
                    lsp -= kRing / 2;
                }
                const uint32_t dn = (uint32_t)(du + 1);
                if (nxt >= 0) {
                    if (lane == 0) ring[(bot + lsp) & (kRing - 1)] = make_uint2((uint32_t)nxt, dn);
                    lsp += 1;
                }
                if (unv && rank < cnt - 1)
                    ring[(bot + lsp + rank) & (kRing - 1)] = make_uint2((uint32_t)v, dn);
                lsp += cnt - 1;
                nxt = read_lane(v, highest_lane(m));
            }
            if (nxt >= 0) {
                u = nxt;
                du += 1;
                continue;
            }
            if (lsp == 0) {
                if (gsp == 0) break;
                const int n = gsp < kRing / 2 ? gsp : kRing / 2;
                // the spill was written by this wave: wait for the stores and
                // drop this CU's L1 copy before reading it back
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                bot = (bot - n) & (kRing - 1);
                for (int i = lane; i < n; i += SDNR_WAVE)
                    ring[(bot + i) & (kRing - 1)] = spill[gsp - n + i];
                gsp -= n;
                lsp = n;
            }
            lsp -= 1;
            const uint2 ent = ring[(bot + lsp) & (kRing - 1)];
            u = uniform((int)ent.x);
            du = uniform((int)ent.y);
        }
        __syncthreads();
        for (int v = lane; v < V; v += SDNR_WAVE) {
            if (((vis[v >> 5] >> (v & 31)) & 1u) == 0u) {
                prow[v] = -1;
                trow[v] = -1;
                if (HOPS) hrow[v] = -1;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Batched pops.  A pop that finds no unvisited neighbour (a "leaf" pop)
// changes nothing -- no mark, no push -- so a run of leaf pops can be checked
// against the same visited set in any order.  The batched kernels read the
// top K stack entries, issue the K row loads and then the K visited gathers
// back to back (one memory latency for K pops instead of K), and take the
// first entry from the top that has an unvisited neighbour: everything above
// it was a leaf pop, it is processed exactly as the sequential search would,
// and everything below stays on the stack for the next batch (its check is
// stale).  On the k=48 fat-tree 96% of pops are leaves.
//
// Rows must fit one wavefront (max out-degree <= 64): ELL rows at u*W, or
// CSR rows (row_ptr loads issued with the batch).  Adjacency arrays carry 64
// padding entries so every lane may load unconditionally (a guarded load per
// batch slot makes hipcc wait vmcnt(0) per slot).
// ---------------------------------------------------------------------------

template <bool ELL, int K>
__device__ __forceinline__ void batch_rows(int kk, const int (&uu)[K], int W,
                                           const int32_t *__restrict__ row_ptr,
                                           const int32_t *__restrict__ col,
                                           int (&rs)[K], int (&v)[K])
{
    // every slot loads unconditionally (addresses stay inside the padded
    // arrays); validity is applied afterwards with bit masks, never with a
    // branch, so the K loads are all in flight together
    const int lane = lane_id();
    int x[K], b[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int u = uu[i];
        if (ELL) {
            rs[i] = u * W;
            b[i] = rs[i] + W;
        } else {
            rs[i] = row_ptr[u];
            b[i] = row_ptr[u + 1];
        }
        x[i] = col[rs[i] + lane];
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int ok = -(int)((i < kk) & (rs[i] + lane < b[i]));   // 0 or -1
        v[i] = (x[i] & ok) | ~ok;
    }
}

// visited test of K candidate rows: K independent LDS gathers, then ballots
template <int K>
__device__ __forceinline__ void batch_unvisited(const uint32_t *vis, const int (&v)[K],
                                                uint64_t (&m)[K])
{
    uint32_t w[K];
#pragma unroll
    for (int i = 0; i < K; ++i) w[i] = vis[(v[i] & 0x7FFFFFFF) >> 5 & ((v[i] >> 31) ^ -1)];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const bool fresh = (v[i] >= 0) & (((w[i] >> (v[i] & 31)) & 1u) == 0u);
        m[i] = __ballot(fresh);
    }
}

template <int K>
__device__ __forceinline__ int first_live(const uint64_t (&m)[K])
{
    int istar = K;
#pragma unroll
    for (int i = K - 1; i >= 0; --i)
        if (m[i] != 0) istar = i;
    return istar;
}

// small graphs (V < 65536): all per-source state in LDS, tables flushed once
template <bool ELL, bool HOPS, int K>
__global__ __launch_bounds__(64) void dfs_lds_batch_kernel(
    int V, int W, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const int32_t *__restrict__ port,
    const int32_t *__restrict__ src, int nsrc, int32_t *__restrict__ out_parent,
    int32_t *__restrict__ out_port, int32_t *__restrict__ out_hops)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int VW = (V + 31) >> 5;
    const int VWp = (VW + 3) & ~3;
    uint32_t *vis = lds;                       // visited bits
    uint32_t *stk = vis + VWp;                 // stack: v | depth << 16
    uint32_t *ps = stk + V;                    // parent | row slot << 16
    uint16_t *dep = reinterpret_cast<uint16_t *>(ps + V);
    const int lane = lane_id();

    for (int si = blockIdx.x; si < nsrc; si += gridDim.x) {
        const int s = uniform(src[si]);
        int32_t *prow = out_parent + (size_t)si * V;
        int32_t *trow = out_port + (size_t)si * V;
        int32_t *hrow = HOPS ? out_hops + (size_t)si * V : nullptr;
        if (s < 0 || s >= V) {
            for (int v = lane; v < V; v += SDNR_WAVE) {
                prow[v] = -1;
                trow[v] = -1;
                if (HOPS) hrow[v] = -1;
            }
            continue;
        }
        for (int w = lane; w < VW; w += SDNR_WAVE) vis[w] = 0u;
        __syncthreads();
        if (lane == 0) {
            vis[s >> 5] = 1u << (s & 31);
            ps[s] = (uint32_t)s;
            dep[s] = 0;
            stk[0] = (uint32_t)s;
        }
        __syncthreads();

        int sp = 1;
        while (sp > 0) {
            const int kk = sp < K ? sp : K;
            const int slot = sp - 1 - lane;
            uint32_t mine = stk[slot < 0 ? 0 : slot];
            mine = lane < kk ? mine : 0u;            // slots past the stack: vertex 0
            uint32_t ent[K];
            int uu[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                ent[i] = (uint32_t)read_lane((int)mine, i);
                uu[i] = (int)(ent[i] & 0xFFFFu);
            }
            int rs[K], v[K];
            batch_rows<ELL, K>(kk, uu, W, row_ptr, col, rs, v);
            uint64_t m[K];
            batch_unvisited<K>(vis, v, m);
            const int istar = first_live<K>(m);
            if (istar == K) {                      // kk leaf pops
                sp -= kk;
                continue;
            }
            sp -= istar + 1;
            uint64_t mm = 0;
            int vv = -1;
            uint32_t eu = 0;
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (i == istar) {
                    mm = m[i];
                    vv = v[i];
                    eu = ent[i];
                }
            const int u = (int)(eu & 0xFFFFu);
            const int du = (int)(eu >> 16);
            if ((mm >> lane) & 1ull) {
                const int rank = lanes_below(mm);
                atomicOr(&vis[vv >> 5], 1u << (vv & 31));
                ps[vv] = (uint32_t)u | ((uint32_t)lane << 16);
                if (HOPS) dep[vv] = (uint16_t)(du + 1);
                stk[sp + rank] = (uint32_t)vv | ((uint32_t)(du + 1) << 16);
            }
            sp += __popcll(mm);
        }
        __syncthreads();

        for (int v = lane; v < V; v += SDNR_WAVE) {
            int p = -1, pt = -1, h = -1;
            if ((vis[v >> 5] >> (v & 31)) & 1u) {
                const uint32_t x = ps[v];
                p = (int)(x & 0xFFFFu);
                if (v == s) {
                    h = 0;
                } else {
                    const int slot = (int)(x >> 16);
                    pt = ELL ? port[(size_t)p * W + slot] : port[row_ptr[p] + slot];
                    h = HOPS ? (int)dep[v] : 0;
                }
            }
            prow[v] = p;
            trow[v] = pt;
            if (HOPS) hrow[v] = h;
        }
        __syncthreads();
    }
}

// large graphs: visited bits + a stack ring in LDS (spilled to HBM in
// halves), table entries stored as vertices are pushed
template <bool ELL, bool HOPS, int K>
__global__ __launch_bounds__(64) void dfs_global_batch_kernel(
    int V, int W, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const int32_t *__restrict__ port,
    const int32_t *__restrict__ src, int nsrc, int32_t *__restrict__ out_parent,
    int32_t *__restrict__ out_port, int32_t *__restrict__ out_hops,
    uint2 *__restrict__ spill_all)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int VW = (V + 31) >> 5;
    const int VWp = (VW + 3) & ~3;
    uint32_t *vis = lds;
    uint2 *ring = reinterpret_cast<uint2 *>(vis + VWp);   // (v, depth)
    uint2 *spill = spill_all + (size_t)blockIdx.x * (size_t)V;
    const int lane = lane_id();

    for (int si = blockIdx.x; si < nsrc; si += gridDim.x) {
        const int s = uniform(src[si]);
        int32_t *prow = out_parent + (size_t)si * V;
        int32_t *trow = out_port + (size_t)si * V;
        int32_t *hrow = HOPS ? out_hops + (size_t)si * V : nullptr;
        if (s < 0 || s >= V) {
            for (int v = lane; v < V; v += SDNR_WAVE) {
                prow[v] = -1;
                trow[v] = -1;
                if (HOPS) hrow[v] = -1;
            }
            continue;
        }
        for (int w = lane; w < VW; w += SDNR_WAVE) vis[w] = 0u;
        __syncthreads();
        if (lane == 0) {
            vis[s >> 5] = 1u << (s & 31);
            prow[s] = s;
            trow[s] = -1;
            if (HOPS) hrow[s] = 0;
            ring[0] = make_uint2((uint32_t)s, 0u);
        }
        __syncthreads();

        int lsp = 1, bot = 0, gsp = 0;        // ring depth, ring bottom, spilled
        for (;;) {
            if (lsp == 0) {
                if (gsp == 0) break;
                const int n = gsp < kRing / 2 ? gsp : kRing / 2;
                // the spill was written by this wave: wait for the stores and
                // drop this CU's L1 copy before reading it back
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                bot = (bot - n) & (kRing - 1);
                for (int i = lane; i < n; i += SDNR_WAVE)
                    ring[(bot + i) & (kRing - 1)] = spill[gsp - n + i];
                gsp -= n;
                lsp = n;
            }
            const int kk = lsp < K ? lsp : K;
            uint2 me = ring[(bot + lsp - 1 - lane) & (kRing - 1)];
            me.x = lane < kk ? me.x : 0u;            // slots past the stack: vertex 0
            me.y = lane < kk ? me.y : 0u;
            uint32_t ent[K], edep[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                ent[i] = (uint32_t)read_lane((int)me.x, i);
                edep[i] = (uint32_t)read_lane((int)me.y, i);
            }
            int uu[K];
#pragma unroll
            for (int i = 0; i < K; ++i) uu[i] = (int)ent[i];
            int rs[K], v[K];
            batch_rows<ELL, K>(kk, uu, W, row_ptr, col, rs, v);
            uint64_t m[K];
            batch_unvisited<K>(vis, v, m);
            const int istar = first_live<K>(m);
            if (istar == K) {
                lsp -= kk;
                continue;
            }
            lsp -= istar + 1;
            uint64_t mm = 0;
            int vv = -1, r0 = 0;
            uint32_t eu = 0, ed = 0;
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (i == istar) {
                    mm = m[i];
                    vv = v[i];
                    eu = ent[i];
                    ed = edep[i];
                    r0 = rs[i];
                }
            const int cnt = __popcll(mm);
            if (lsp + cnt > kRing) {               // spill the oldest half
                for (int i = lane; i < kRing / 2; i += SDNR_WAVE)
                    spill[gsp + i] = ring[(bot + i) & (kRing - 1)];
                gsp += kRing / 2;
                bot = (bot + kRing / 2) & (kRing - 1);
                lsp -= kRing / 2;
            }
            if ((mm >> lane) & 1ull) {
                const int rank = lanes_below(mm);
                atomicOr(&vis[vv >> 5], 1u << (vv & 31));
                prow[vv] = (int)eu;
                trow[vv] = port[r0 + lane];
                if (HOPS) hrow[vv] = (int)ed + 1;
                ring[(bot + lsp + rank) & (kRing - 1)] = make_uint2((uint32_t)vv, ed + 1u);
            }
            lsp += cnt;
        }
        __syncthreads();
        for (int v = lane; v < V; v += SDNR_WAVE) {
            if (((vis[v >> 5] >> (v & 31)) & 1u) == 0u) {
                prow[v] = -1;
                trow[v] = -1;
                if (HOPS) hrow[v] = -1;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Cooperative batched pops (small graphs, the k=48 headline path).
//
// With one wavefront per source the batched loop is instruction-issue bound
// (one wave per SIMD pays >= 4 cycles per instruction on the chain).  Here a
// workgroup of NW waves owns one source: each wave checks KW of the K = NW*KW
// top stack entries (row load + visited gather + ballot), publishes one flag
// word per wave, and after one barrier every wave derives the same first
// live slot; the owning wave pushes, and a second barrier publishes the push
// (skipped when all K entries were leaf pops).  Rows are u16 with stride 64
// (one 128-byte line each) padded with a sentinel vertex V whose visited bit
// is always set, and row V is all sentinel: no lane or slot needs a validity
// mask.  Every wave keeps its own copy of the stack depth; all copies follow
// the same deterministic updates.
// ---------------------------------------------------------------------------
template <int NW, int KW, bool HOPS>
__global__ __launch_bounds__(NW * 64) void dfs_coop_kernel(
    int V, const uint16_t *__restrict__ adj, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ port, const int32_t *__restrict__ src, int nsrc,
    int32_t *__restrict__ out_parent, int32_t *__restrict__ out_port,
    int32_t *__restrict__ out_hops)
{
    constexpr int K = NW * KW;
    static_assert(K <= 64, "one flag bit per slot");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int VW = (V + 1 + 31) >> 5;            // + sentinel bit V
    const int VWp = (VW + 3) & ~3;
    uint32_t *vis = lds;
    uint32_t *stk = vis + VWp;                   // v | depth << 16
    uint32_t *ps = stk + V;                      // parent | row slot << 16
    uint16_t *dep = reinterpret_cast<uint16_t *>(ps + V);
    uint32_t *xch = ps + V + ((V + 1) >> 1);     // flags[2][NW], count[2]
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;

    for (int si = blockIdx.x; si < nsrc; si += gridDim.x) {
        const int s = uniform(src[si]);
        int32_t *prow = out_parent + (size_t)si * V;
        int32_t *trow = out_port + (size_t)si * V;
        int32_t *hrow = HOPS ? out_hops + (size_t)si * V : nullptr;
        if (s < 0 || s >= V) {
            for (int v = threadIdx.x; v < V; v += blockDim.x) {
                prow[v] = -1;
                trow[v] = -1;
                if (HOPS) hrow[v] = -1;
            }
            continue;
        }
        for (int i = threadIdx.x; i < VW; i += blockDim.x) vis[i] = 0u;
        __syncthreads();
        if (threadIdx.x == 0) {
            vis[s >> 5] |= 1u << (s & 31);
            vis[V >> 5] |= 1u << (V & 31);
            ps[s] = (uint32_t)s;
            dep[s] = 0;
            stk[0] = (uint32_t)s;
        }
        __syncthreads();

        int sp = 1, par = 0;
        while (sp > 0) {
            const int kk = sp < K ? sp : K;
            const int slot = w * KW + lane;
            const int at = sp - 1 - slot;
            uint32_t mine = stk[at < 0 ? 0 : at];
            mine = slot < kk ? mine : (uint32_t)V;          // past the stack: sentinel row
            uint32_t ent[KW];
            int x[KW];
#pragma unroll
            for (int j = 0; j < KW; ++j) ent[j] = (uint32_t)read_lane((int)mine, j);
#pragma unroll
            for (int j = 0; j < KW; ++j) {
                const uint16_t *row = adj + (size_t)(ent[j] & 0xFFFFu) * 64;
                x[j] = row[lane];
            }
            uint32_t wd[KW];
#pragma unroll
            for (int j = 0; j < KW; ++j) wd[j] = vis[x[j] >> 5];
            uint64_t m[KW];
            uint32_t fl = 0;
#pragma unroll
            for (int j = 0; j < KW; ++j) {
                m[j] = __ballot(((wd[j] >> (x[j] & 31)) & 1u) == 0u);
                fl |= (m[j] != 0 ? 1u : 0u) << j;
            }
            if (lane == 0) xch[par * NW + w] = fl;
            __syncthreads();
            const uint32_t fw = xch[par * NW + (lane < NW ? lane : 0)];
            uint64_t gm = 0;
#pragma unroll
            for (int q = 0; q < NW; ++q) gm |= (uint64_t)(uint32_t)read_lane((int)fw, q) << (q * KW);
            if (gm == 0) {                               // K leaf pops
                sp -= kk;
                par ^= 1;
                continue;
            }
            const int istar = __ffsll((unsigned long long)gm) - 1;
            sp -= istar + 1;
            if (w == istar / KW) {
                const int js = istar % KW;
                uint64_t mm = 0;
                int xv = 0;
                uint32_t eu = 0;
#pragma unroll
                for (int j = 0; j < KW; ++j)
                    if (j == js) {
                        mm = m[j];
                        xv = x[j];
                        eu = ent[j];
                    }
                const int u = (int)(eu & 0xFFFFu);
                const uint32_t dn = (eu >> 16) + 1u;
                if ((mm >> lane) & 1ull) {
                    atomicOr(&vis[xv >> 5], 1u << (xv & 31));
                    ps[xv] = (uint32_t)u | ((uint32_t)lane << 16);
                    if (HOPS) dep[xv] = (uint16_t)dn;
                    stk[sp + lanes_below(mm)] = (uint32_t)xv | (dn << 16);
                }
                if (lane == 0) xch[2 * NW + par] = (uint32_t)__popcll(mm);
            }
            __syncthreads();
            sp += (int)xch[2 * NW + par];
            par ^= 1;
        }
        __syncthreads();

        for (int v = threadIdx.x; v < V; v += blockDim.x) {
            int p = -1, pt = -1, h = -1;
            if ((vis[v >> 5] >> (v & 31)) & 1u) {
                const uint32_t xx = ps[v];
                p = (int)(xx & 0xFFFFu);
                if (v == s) {
                    h = 0;
                } else {
                    pt = port[row_ptr[p] + (int)(xx >> 16)];
                    h = HOPS ? (int)dep[v] : 0;
                }
            }
            prow[v] = p;
            trow[v] = pt;
            if (HOPS) hrow[v] = h;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Counted pops (small graphs with in/out-degree <= 64): the k=48 headline.
//
// cnt[u] = number of out-neighbours of u not yet visited.  A pop is a leaf
// pop exactly when cnt[u] == 0, so runs of leaf pops are skipped 64 stack
// entries at a time: one LDS read of the stack slots, one gather of their
// counts, one ballot -- no adjacency row is touched.  The price is moved to
// push time, where it is parallel: a vertex v that becomes visited
// decrements cnt[x] for every in-neighbour x (its reverse row, loaded with
// the other children's rows in flight together, then ds_sub_u32 on packed
// u16 pairs -- a count never drops below zero, so no borrow crosses halves).
// Only the non-leaf pops (~4% on the k=48 fat-tree) load a forward row and
// gather visited bits.  A workgroup of NW waves owns one source: every wave
// runs the skip and the row check redundantly (same LDS state, same result,
// no exchange), wave 0 writes marks/stack/tree, the children's decrements
// are split round-robin over the waves; barrier A separates the visited
// gathers from the marks, barrier B publishes the push.
// ---------------------------------------------------------------------------
#ifdef SDNR_STAMPS
// diagnostic build only: cycles per phase of the counted-pop loop, summed
// over every source by wave 0 of each workgroup (never in the real kernel)
__device__ unsigned long long g_stamp[16];
#define SDNR_STAMP(t) \
    do { __builtin_amdgcn_sched_barrier(0); \
         asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory"); \
         __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define SDNR_STAMP(t) do { (void)(t); } while (0)
#endif

template <int NW, bool HOPS>
__global__ __launch_bounds__(NW * 64) void dfs_count_kernel(
    int V, const uint16_t *__restrict__ adj, const uint16_t *__restrict__ radj,
    const uint32_t *__restrict__ deg, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ port, const int32_t *__restrict__ src, int nsrc,
    int32_t *__restrict__ out_parent, int32_t *__restrict__ out_port,
    int32_t *__restrict__ out_hops)
{
    constexpr int G = 8;                         // child rows in flight per wave
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int VW = (V + 1 + 31) >> 5;            // + sentinel bit V
    const int VWp = (VW + 3) & ~3;
    const int CWp = (V + 1 + 3) & ~3;            // u32 counts of 0..V
    const int SWp = (((V + 1) >> 1) + 3) & ~3;   // u16 stack
    uint32_t *vis = lds;
    uint32_t *cnt = vis + VWp;
    uint16_t *stk = reinterpret_cast<uint16_t *>(cnt + CWp);
    uint32_t *ps = cnt + CWp + SWp;              // parent | row slot << 16
    uint16_t *dep = reinterpret_cast<uint16_t *>(ps + V);
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;   // stamps (diag)
#ifdef SDNR_STAMPS
    unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
#endif

    for (int si = blockIdx.x; si < nsrc; si += gridDim.x) {
        const int s = uniform(src[si]);
        int32_t *prow = out_parent + (size_t)si * V;
        int32_t *trow = out_port + (size_t)si * V;
        int32_t *hrow = HOPS ? out_hops + (size_t)si * V : nullptr;
        if (s < 0 || s >= V) {
            for (int v = threadIdx.x; v < V; v += blockDim.x) {
                prow[v] = -1;
                trow[v] = -1;
                if (HOPS) hrow[v] = -1;
            }
            continue;
        }
        for (int i = threadIdx.x; i < VW; i += blockDim.x) vis[i] = 0u;
        for (int i = threadIdx.x; i <= V; i += blockDim.x) cnt[i] = deg[i];
        __syncthreads();
        if (threadIdx.x == 0) {
            vis[s >> 5] |= 1u << (s & 31);
            vis[V >> 5] |= 1u << (V & 31);
            ps[s] = (uint32_t)s;
            if (HOPS) dep[s] = 0;
            stk[0] = (uint16_t)s;
        }
        if (w == 0) {                            // s is visited: its in-neighbours lose one
            const int r = radj[(size_t)s * 64 + lane];
            if (r != V) atomicSub(&cnt[r], 1u);
        }
        __syncthreads();

        int sp = 1;
        int pu = -1, xpre = V;                   // speculatively loaded row of pu
        for (;;) {
            SDNR_STAMP(t0);
            // ---- skip leaf pops, 64 stack slots per step
            uint64_t m = 0;
            int e = V;
            while (sp > 0) {
                const int kk = sp < 64 ? sp : 64;
                const int at = sp - 1 - lane;
                e = stk[at < 0 ? 0 : at];
                e = lane < kk ? e : V;
                m = __ballot(cnt[e] != 0u);
                if (m) break;
                sp -= kk;
            }
            if (!m) break;
            const int first = __ffsll((unsigned long long)m) - 1;
            const int u = read_lane(e, first);
            sp -= first + 1;
            SDNR_STAMP(t1);
            // ---- the non-leaf pop: forward row (usually prefetched: the
            // top of the stack is the previous push's largest child), visited gather
            const int x = (u == pu) ? xpre : (int)adj[(size_t)u * 64 + lane];
            const uint32_t wv = vis[x >> 5];
            const bool fresh = ((wv >> (x & 31)) & 1u) == 0u;
            const uint64_t mm = __ballot(fresh);
            const int rank = lanes_below(mm);
            pu = read_lane(x, highest_lane(mm));     // cnt[u] != 0 -> mm != 0
            xpre = adj[(size_t)pu * 64 + lane];
            int du = 0;
            if (HOPS) du = uniform((int)dep[u]);
            SDNR_STAMP(t2);
            __syncthreads();                     // A: gathers before marks
            SDNR_STAMP(t3);
            if (w == 0 && fresh) {
                atomicOr(&vis[x >> 5], 1u << (x & 31));
                ps[x] = (uint32_t)u | ((uint32_t)lane << 16);
                if (HOPS) dep[x] = (uint16_t)(du + 1);
                stk[sp + rank] = (uint16_t)x;
            }
            // ---- children decrement their in-neighbours' counts; child j
            // (ascending) belongs to wave j % NW, up to G rows in flight
            uint64_t mine = __ballot(fresh && (rank % NW) == w);
            int n = __popcll(mine);
            while (n > 0) {
                int r[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    int v = V;                   // past n: the all-sentinel row
                    if (g < n) {
                        v = read_lane(x, __ffsll((unsigned long long)mine) - 1);
                        mine &= mine - 1;
                    }
                    r[g] = radj[(size_t)v * 64 + lane];
                }
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (g < n && r[g] != V) atomicSub(&cnt[r[g]], 1u);
                n -= G;
            }
            sp += __popcll(mm);
            SDNR_STAMP(t4);
            __syncthreads();                     // B: publish the push
            SDNR_STAMP(t5);
#ifdef SDNR_STAMPS
            acc[0] += t1 - t0;
            acc[1] += t2 - t1;
            acc[2] += t3 - t2;
            acc[3] += t4 - t3;
            acc[4] += t5 - t4;
            acc[5] += 1;
#endif
        }
        __syncthreads();

        for (int v = threadIdx.x; v < V; v += blockDim.x) {
            int p = -1, pt = -1, h = -1;
            if ((vis[v >> 5] >> (v & 31)) & 1u) {
                const uint32_t xx = ps[v];
                p = (int)(xx & 0xFFFFu);
                if (v == s) {
                    h = 0;
                } else {
                    pt = port[row_ptr[p] + (int)(xx >> 16)];
                    h = HOPS ? (int)dep[v] : 0;
                }
            }
            prow[v] = p;
            trow[v] = pt;
            if (HOPS) hrow[v] = h;
        }
        __syncthreads();
    }
#ifdef SDNR_STAMPS
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) atomicAdd(&g_stamp[k], acc[k]);
#endif
}

// ---------------------------------------------------------------------------
// Lane-packed batched pops for large, low-degree graphs (torus 32^3: 6,
// Jellyfish: 16).  A row needs only LPR >= W lanes, so one wave instruction
// checks R = 64/LPR stack entries (lane l -> slot l/LPR, row position l%LPR)
// and J instructions check K = R*J entries: R times fewer loads, gathers and
// ballots per pop than one-row-per-wavefront.  Same exact semantics as
// dfs_global_batch_kernel (first live entry from the top is processed).
// ---------------------------------------------------------------------------
template <int LPR, int J, bool HOPS, int RING>
__global__ __launch_bounds__(64) void dfs_global_packed_kernel(
    int V, int W, const int32_t *__restrict__ col, const int32_t *__restrict__ port,
    const int32_t *__restrict__ src, int nsrc, int32_t *__restrict__ out_parent,
    int32_t *__restrict__ out_port, int32_t *__restrict__ out_hops,
    uint2 *__restrict__ spill_all)
{
    constexpr int R = 64 / LPR;
    constexpr int K = R * J;
    static_assert(K <= 64, "one stack slot per lane");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int VW = (V + 31) >> 5;
    const int VWp = (VW + 3) & ~3;
    uint32_t *vis = lds;
    uint2 *ring = reinterpret_cast<uint2 *>(vis + VWp);   // (v, depth)
    uint2 *spill = spill_all + (size_t)blockIdx.x * (size_t)V;
    const int lane = lane_id();
    const int pos = lane % LPR;
    const int sub = lane / LPR;
    const uint64_t lowmask = (LPR == 64) ? ~0ull : ((1ull << LPR) - 1ull);

    for (int si = blockIdx.x; si < nsrc; si += gridDim.x) {
        const int s = uniform(src[si]);
        int32_t *prow = out_parent + (size_t)si * V;
        int32_t *trow = out_port + (size_t)si * V;
        int32_t *hrow = HOPS ? out_hops + (size_t)si * V : nullptr;
        if (s < 0 || s >= V) {
            for (int v = lane; v < V; v += SDNR_WAVE) {
                prow[v] = -1;
                trow[v] = -1;
                if (HOPS) hrow[v] = -1;
            }
            continue;
        }
        for (int w = lane; w < VW; w += SDNR_WAVE) vis[w] = 0u;
        __syncthreads();
        if (lane == 0) {
            vis[s >> 5] = 1u << (s & 31);
            prow[s] = s;
            trow[s] = -1;
            if (HOPS) hrow[s] = 0;
            ring[0] = make_uint2((uint32_t)s, 0u);
        }
        __syncthreads();

        int lsp = 1, bot = 0, gsp = 0;
        for (;;) {
            if (lsp == 0) {
                if (gsp == 0) break;
                const int n = gsp < RING / 2 ? gsp : RING / 2;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                bot = (bot - n) & (RING - 1);
                for (int i = lane; i < n; i += SDNR_WAVE)
                    ring[(bot + i) & (RING - 1)] = spill[gsp - n + i];
                gsp -= n;
                lsp = n;
            }
            const int kk = lsp < K ? lsp : K;
            uint2 me = ring[(bot + lsp - 1 - lane) & (RING - 1)];
            me.x = lane < kk ? me.x : 0u;
            me.y = lane < kk ? me.y : 0u;
            int x[J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int slot = j * R + sub;
                const int u = __shfl((int)me.x, slot);             // slot >= kk: vertex 0
                x[j] = col[u * W + pos];
            }
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int ok = -(int)(((j * R + sub) < kk) & (pos < W));
                x[j] = (x[j] & ok) | ~ok;
            }
            uint64_t m[J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int xi = x[j] & 0x7FFFFFFF;
                const uint32_t w = vis[(xi >> 5) & ((x[j] >> 31) ^ -1)];
                m[j] = __ballot((x[j] >= 0) & (((w >> (xi & 31)) & 1u) == 0u));
            }
            int jstar = J;
#pragma unroll
            for (int j = J - 1; j >= 0; --j)
                if (m[j] != 0) jstar = j;
            if (jstar == J) {
                lsp -= kk;
                continue;
            }
            uint64_t mj = 0;
            int vv = -1;
#pragma unroll
            for (int j = 0; j < J; ++j)
                if (j == jstar) {
                    mj = m[j];
                    vv = x[j];
                }
            const int sstar = (__ffsll((unsigned long long)mj) - 1) / LPR;   // sub-slot
            const int istar = jstar * R + sstar;
            const uint64_t mm = mj & (lowmask << (sstar * LPR));
            const int eu = read_lane((int)me.x, istar);
            const uint32_t ed = (uint32_t)read_lane((int)me.y, istar);
            lsp -= istar + 1;
            const int cnt = __popcll(mm);
            if (lsp + cnt > RING) {
                for (int i = lane; i < RING / 2; i += SDNR_WAVE)
                    spill[gsp + i] = ring[(bot + i) & (RING - 1)];
                gsp += RING / 2;
                bot = (bot + RING / 2) & (RING - 1);
                lsp -= RING / 2;
            }
            if ((mm >> lane) & 1ull) {
                const int rank = lanes_below(mm);
                atomicOr(&vis[vv >> 5], 1u << (vv & 31));
                prow[vv] = eu;
                trow[vv] = port[eu * W + pos];
                if (HOPS) hrow[vv] = (int)ed + 1;
                ring[(bot + lsp + rank) & (RING - 1)] = make_uint2((uint32_t)vv, ed + 1u);
            }
            lsp += cnt;
        }
        __syncthreads();
        for (int v = lane; v < V; v += SDNR_WAVE) {
            if (((vis[v >> 5] >> (v & 31)) & 1u) == 0u) {
                prow[v] = -1;
                trow[v] = -1;
                if (HOPS) hrow[v] = -1;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Search / writer split for large graphs (torus 32^3, Jellyfish 100k).
//
// rocprofv3 on dfs_global_packed_kernel (profiles/r02_torus_dfs_*,
// r02_jf_dfs_*): 84% / 64% of wave cycles waiting.  That kernel stores the
// table entries (parent, port) from the search wave at every push, and a
// wave's vector-memory counter is in order: the next row load's wait also
// waits for every table store issued before it -- a write acknowledgement on
// each step of the serial chain -- and the port lookup sits on the chain
// too.  Here NS search waves of a workgroup (one source each) never store on
// the chain: a push appends (vertex, parent, row slot[, depth]) records to
// the wave's LDS queue and a writer wave drains the NS queues, loads the
// ports and issues the table stores (parent | port << 16 directly when the
// packed layout is asked for).  Rows are read in the narrowest format the
// vertex count allows -- u16 ids below 65,535 vertices; 16 low bits plus a
// per-row mask of the 17th bit below 131,071 (the 100k Jellyfish ELL drops
// from 6.4 MB to 3.6 MB, inside an XCD's 4 MB L2).  The search itself is the
// batched pop of dfs_global_packed_kernel (first live entry from the top).
// ---------------------------------------------------------------------------
constexpr int kRow32 = 0, kRow16 = 1, kRow17 = 2;
// dictionary rows (split kernel, rows of <= 8 slots): row u = u + D[p(u)],
// the pattern ids and D staged in LDS (capi.hip upload_dict)
constexpr int kRowDict = 3;
constexpr int kSplitQ = 64;                    // queued records per search wave
// SDNROUTE_DFS_FLAGS (tuning): search waves at raised issue priority,
// non-temporal table stores, or (diagnostic) no table stores at all / port
// slot instead of the port
// (diagnostic) no port lookups in the writer
constexpr int kFlagPrio = 1, kFlagNT = 2, kFlagNoStore = 4, kFlagNoPort = 8;
// dfs_async_kernel: the worker rows are pre-swizzled count indices (radjw)
constexpr int kFlagPreSwz = 16;
// hop counts written as u16 (0xFFFF unreached) instead of int32: the depth
// plane of the drop-in's table pool (sdnr_dfs_tables_tree)
constexpr int kFlagHops16 = 32;
// split kernel: sources taken from the CU's own contiguous chunk (see
// split_next_source) instead of the static blockIdx-strided order
constexpr int kFlagCuMap = 64;
// async kernel: when every fresh child of a candidate is a leaf, the next
// candidate comes off the stack -- read its window, counts and row before
// the push instead of after it
constexpr int kFlagSpecPop = 128;

// s_getreg encodings: (size - 1) << 11 | offset << 6 | register id
constexpr int kHwIdReg = (31 << 11) | 4;      // HW_REG_HW_ID: cu [11:8], sh [12], se [14:13]
constexpr int kXccIdReg = (15 << 11) | 20;    // HW_REG_XCC_ID: the XCD

// Number of this wave's CU, 0, 1, 2, ... in order of first arrival (wq:
// [nch] chunk cursors | arrivals counter | 1,024-entry CU table, -1 = not
// numbered yet, -2 = being numbered).  Lane 0 works; the result is uniform.
__device__ int split_cu_number(int *wq, int nch, int lane, int *err)
{
    const uint32_t hw = __builtin_amdgcn_s_getreg(kHwIdReg);
    const uint32_t xcc = __builtin_amdgcn_s_getreg(kXccIdReg) & 7u;
    const int key = (int)((((xcc * 4u + ((hw >> 13) & 3u)) * 2u + ((hw >> 12) & 1u)) * 16u) +
                          ((hw >> 8) & 15u));
    int *tab = wq + nch + 1;
    int n = 0;
    if (lane == 0) {
        int v = atomicCAS(&tab[key], -1, -2);
        if (v == -1) {
            n = atomicAdd(&wq[nch], 1);
            __hip_atomic_store(&tab[key], n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            for (unsigned spin = 0; v < 0; ++spin) {
                if (spin > (1u << 22)) {
                    atomicOr(err, 32);
                    v = 0;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
                v = __hip_atomic_load(&tab[key], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            }
            n = v;
        }
    }
    return uniform(read_lane(n, 0)) % nch;
}

// The next source of a search wave under kFlagCuMap: the sources are cut
// into nch contiguous chunks, one per CU (by arrival number); a wave takes
// the next source of its chunk, so the ~28 search waves co-resident on a CU
// walk neighbouring sources at the same time (on the torus their traversals
// read neighbouring rows, which the CU's L1 then serves).  A
// wave whose chunk is exhausted looks 64 chunks at a time for one with
// sources left (cursor loads at agent scope) and takes from it.  Returns
// nsrc when no chunk has work.  Bounded: every failed claim exhausts a chunk.
__device__ int split_next_source(int *wq, int nch, int nsrc, int *chunk, int lane)
{
    for (int guard = 0; guard <= 2 * nch + 2; ++guard) {
        const int c = *chunk;
        const int lo = (int)((int64_t)c * nsrc / nch), hi = (int)((int64_t)(c + 1) * nsrc / nch);
        int t = 0;
        if (lane == 0) t = atomicAdd(&wq[c], 1);
        t = uniform(read_lane(t, 0));
        if (lo + t < hi) return lo + t;
        int found = -1;
        for (int base = 0; base < nch && found < 0; base += SDNR_WAVE) {
            const int k = base + lane;
            bool has = false;
            int cc = 0;
            if (k < nch) {
                cc = c + 1 + k < nch ? c + 1 + k : c + 1 + k - nch;
                const int l2 = (int)((int64_t)cc * nsrc / nch);
                const int h2 = (int)((int64_t)(cc + 1) * nsrc / nch);
                has = l2 + __hip_atomic_load(&wq[cc], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < h2;
            }
            const uint64_t m = __ballot(has);
            if (m) found = read_lane(cc, __ffsll((unsigned long long)m) - 1);
        }
        if (found < 0) return nsrc;
        *chunk = found;
    }
    return nsrc;
}

// hop count of entry e of an [rows][V] hop table, int32 or u16 (kFlagHops16)
__device__ __forceinline__ void put_hop(int32_t *__restrict__ hops, size_t e, int h, int flags)
{
    if (flags & kFlagHops16) reinterpret_cast<uint16_t *>(hops)[e] = (uint16_t)h;
    else hops[e] = h;
}

template <int FMT>
__device__ __forceinline__ int split_row(const void *__restrict__ rows,
                                         const uint32_t *__restrict__ rhi, int V, int W, int u,
                                         int pos)
{
    const size_t e = (size_t)u * W + pos;
    int x;
    if (FMT == kRow32) {
        x = static_cast<const int32_t *>(rows)[e];
    } else {
        x = (int)static_cast<const uint16_t *>(rows)[e];
        if (FMT == kRow17) x |= (int)((rhi[u] >> pos) & 1u) << 16;
    }
    return x < V ? x : -1;                     // padding (-1, 0xFFFF, 0x1FFFF)
}

// visited-bit word w lives at w ^ ((w >> 5) & 31): words 32 apart (ids 1,024
// apart -- a 32^3 torus's z neighbours) fall in different LDS banks
__device__ __forceinline__ int vsw(int w) { return w ^ ((w >> 5) & 31); }

// stack ring entries: (vertex, depth), or the vertex alone (half the LDS:
// more sources per CU on the 100k Jellyfish, 10 instead of 9; measured 13 %
// slower on the torus, which keeps the pair)
template <bool HOPS> struct SplitRing;
template <> struct SplitRing<true> {
    using T = uint2;
    static __device__ __forceinline__ uint2 get(T e) { return e; }
    static __device__ __forceinline__ T put(uint32_t v, uint32_t d) { return make_uint2(v, d); }
};
template <> struct SplitRing<false> {
    using T = uint32_t;
    static __device__ __forceinline__ uint2 get(T e) { return make_uint2(e, 0u); }
    static __device__ __forceinline__ T put(uint32_t v, uint32_t) { return v; }
};

// dictionary rows without hop counts: one u32 per entry, vertex | pattern
// << 16 (V <= 65535) -- the narrow ring keeps the 32^3 torus at 4 workgroups
// per CU with the dictionary's LDS added
struct SplitRingDict {
    using T = uint32_t;
    static __device__ __forceinline__ uint2 get(T e) { return make_uint2(e & 0xFFFFu, e >> 16); }
    static __device__ __forceinline__ T put(uint32_t v, uint32_t y) { return v | (y << 16); }
};

__host__ __device__ constexpr bool split_wide_ring(int lpr, bool hops, bool dict = false)
{
    return hops || (lpr == 8 && !dict);
}

__host__ __device__ inline size_t split_lds_words(int V, int ring, int ns, bool hops, int lpr,
                                                  bool dict = false)
{
    const size_t VWp = (size_t)((((V + 31) >> 5) + 31) & ~31);
    return (size_t)ns * (VWp + (split_wide_ring(lpr, hops, dict) ? 2 : 1) * (size_t)ring) +
           (size_t)ns * kSplitQ * (hops ? 3 : 2) +
           ((3 * (size_t)ns + 3) & ~(size_t)3);
}

// tree layouts of the split kernel: int32 parent/port tables, parent | port
// << 16 (sdnr_dfs_tables_packed), parent | slot << 26 (sdnr_dfs_tables_slots)
constexpr int kTreeInt32 = 0, kTreePort16 = 1, kTreeSlot = 2;

// The writer wave of the split kernels: drains the NS search waves' record
// queues (vertex | slot << 26, parent[, depth]) into the table rows, loading
// the port of each tree edge off the search chain.  One round takes the
// records of ALL queues at once, packed into the 64 lanes (queue k's pending
// records after queue k-1's), so a round is one LDS read -> port load ->
// store chain however many queues have records (round 5 drained the queues
// one after the other: NS dependent port-load round trips per round, and
// with dictionary rows -- a search twice as fast -- the search waves then
// waited 929 cycles per push for queue room; stamps).
template <int NS, bool HOPS, int PK>
__device__ __forceinline__ void split_writer(int V, int W, const int32_t *__restrict__ ell_port,
                                             const uint2 *qrec, const uint32_t *qdep, int *ctl,
                                             int lane, int32_t *__restrict__ out_parent,
                                             int32_t *__restrict__ out_port,
                                             int32_t *__restrict__ out_hops, int *__restrict__ err,
                                             int flags)
{
    static_assert(NS <= 32, "one lane per queue");
    constexpr unsigned kIdle = 1u << 26;
    constexpr bool PACKED = PK != kTreeInt32;
    int consd = 0;                     // lane k < NS: records of queue k consumed
    unsigned idle = 0;
    for (;;) {
        // records first, then the row: a source's row is announced before
        // its first record, and changes only after the writer consumed all
        // of the previous source's records
        int P = 0, row = -1;
        if (lane < NS) {
            P = __hip_atomic_load(&ctl[lane], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            row = __hip_atomic_load(&ctl[2 * NS + lane], __ATOMIC_ACQUIRE,
                                    __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        const int avail = lane < NS ? P - consd : 0;
        // exclusive prefix of the queues' pending records over lanes 0..NS-1
        int incl = avail;
#pragma unroll
        for (int d = 1; d < NS; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const int excl = incl - avail;
        const int total = read_lane(incl, NS - 1);
        if (total > 0) {
            // lane l serves record l of the packed list: queue k with
            // excl_k <= l < excl_k + avail_k (a uniform scan over the queues)
            int k = -1, idx = 0, crow = 0, cbase = 0;
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const int e = read_lane(excl, q), a = read_lane(avail, q);
                if (lane >= e && lane < e + a) {
                    k = q;
                    idx = lane - e;
                    crow = read_lane(row, q);
                    cbase = read_lane(consd, q);
                }
            }
            if (k >= 0) {
                const int at = k * kSplitQ + ((cbase + idx) & (kSplitQ - 1));
                const uint2 r = qrec[at];
                const int v = (int)(r.x & 0x3FFFFFFu), slot = (int)(r.x >> 26);
                const int par = (int)r.y;
                const size_t e = (size_t)crow * V + v;
                if (PK == kTreeSlot) {         // no port lookup: the slot names it
                    const int32_t tv = (int32_t)((uint32_t)par | ((uint32_t)slot << 26));
                    if (flags & kFlagNT) __builtin_nontemporal_store(tv, &out_parent[e]);
                    else if (!(flags & kFlagNoStore)) out_parent[e] = tv;
                    if (HOPS && !(flags & kFlagNoStore)) put_hop(out_hops, e, (int)qdep[at], flags);
                } else {
                    const int pt = (flags & kFlagNoPort) ? slot : ell_port[(size_t)par * W + slot];
                    if (flags & kFlagNoStore) {
                        // diagnostic: records consumed, no table stores
                    } else if (flags & kFlagNT) {
                        if (PACKED) {
                            __builtin_nontemporal_store(
                                (int32_t)(((uint32_t)par & 0xFFFFu) | ((uint32_t)pt << 16)),
                                &out_parent[e]);
                        } else {
                            __builtin_nontemporal_store(par, &out_parent[e]);
                            __builtin_nontemporal_store(pt, &out_port[e]);
                        }
                        if (HOPS) {
                            if (flags & kFlagHops16)
                                __builtin_nontemporal_store(
                                    (uint16_t)qdep[at], reinterpret_cast<uint16_t *>(out_hops) + e);
                            else
                                __builtin_nontemporal_store((int)qdep[at], &out_hops[e]);
                        }
                    } else {
                        if (PACKED) {
                            out_parent[e] = (int32_t)(((uint32_t)par & 0xFFFFu) |
                                                      ((uint32_t)pt << 16));
                        } else {
                            out_parent[e] = par;
                            out_port[e] = pt;
                        }
                        if (HOPS) put_hop(out_hops, e, (int)qdep[at], flags);
                    }
                }
            }
            // queue k's share of this round (the list is cut at 64 lanes)
            const int took = lane < NS ? max(0, min(avail, SDNR_WAVE - excl)) : 0;
            consd += took;
            // the record reads above are done (LDS ops in order)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            if (took > 0) __hip_atomic_store(&ctl[NS + lane], consd, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_WORKGROUP);
            idle = 0;
            continue;
        }
        // nothing pending: done when every queue's wave has finished (row
        // -1) and published nothing meanwhile
        bool done = true;
        if (lane < NS)
            done = row == -1 && __hip_atomic_load(&ctl[lane], __ATOMIC_ACQUIRE,
                                                  __HIP_MEMORY_SCOPE_WORKGROUP) == consd;
        if (__ballot(!done) == 0ull) break;
        if (++idle > kIdle) {
            if (lane == 0) atomicOr(err, 16);
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

template <int LPR, int J, bool HOPS, int RING, int NS, int FMT, int PK>
__global__ __launch_bounds__((NS + 1) * 64) void dfs_split_kernel(
    int V, int W, const void *__restrict__ rows, const uint32_t *__restrict__ rhi,
    const int32_t *__restrict__ ell_port, const int32_t *__restrict__ src, int nsrc,
    int32_t *__restrict__ out_parent, int32_t *__restrict__ out_port,
    int32_t *__restrict__ out_hops, uint2 *__restrict__ spill_all, int *__restrict__ err,
    int flags, int *__restrict__ wq, int nch, const uint32_t *__restrict__ dict_bp,
    const uint32_t *__restrict__ dict_bt, const int32_t *__restrict__ dict_off, int dict_bpw,
    int dict_NB, int dict_P)
{
    // kRowDict: a stack entry carries its vertex's pattern id (ring .y =
    // pattern | depth << 8), a window's row is u + D[pattern][slot] from LDS
    // and the new children's pattern ids (two dictionary levels, capi.hip
    // upload_dict) are read beside their visited words, so the chain touches
    // no global memory (the torus's window was one dependent
    // L2 row read at the loaded L2 latency)
    constexpr bool DICT = FMT == kRowDict;
    static_assert(!DICT || LPR == 8, "dictionary rows: 8 lanes per row");
    constexpr int R = 64 / LPR;
    constexpr int K = R * J;
    constexpr unsigned kSpin = 1u << 22;
    constexpr bool PACKED = PK != kTreeInt32;
    static_assert(K <= 64, "one stack slot per lane");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int VW = (V + 31) >> 5;
    const int VWp = (VW + 31) & ~31;          // whole 32-word blocks (swizzled)
    constexpr bool WR = split_wide_ring(LPR, HOPS, DICT);
    // entries carry (vertex, y): y = depth, or with dictionary rows the
    // pattern id (| depth << 8 with hop counts: the wide ring)
    constexpr bool YR = WR || DICT;
    using RE = typename std::conditional<DICT && !WR, SplitRingDict, SplitRing<WR>>::type;
    using RT = typename RE::T;
    const int per = VWp + (WR ? 2 : 1) * RING;   // words per search wave: vis | stack ring
    uint2 *qrec = reinterpret_cast<uint2 *>(lds + NS * per);
    uint32_t *qdep = reinterpret_cast<uint32_t *>(qrec + NS * kSplitQ);
    // ctl[k] records published by search wave k, ctl[NS + k] records the
    // writer consumed, ctl[2NS + k] table row of wave k's source (-2 none
    // yet, -1 no more)
    int *ctl = reinterpret_cast<int *>(qdep + (HOPS ? NS * kSplitQ : 0));
    // dictionary: block ids (4 per word), block tuples (8 words each), then
    // D (8 offsets per pattern id)
    uint32_t *lbp = reinterpret_cast<uint32_t *>(ctl) + ((3 * NS + 3) & ~3);
    uint32_t *lbt = lbp + (DICT ? dict_bpw : 0);
    const int32_t *loff = reinterpret_cast<const int32_t *>(lbt + (DICT ? 8 * dict_NB : 0));
    const int lane = lane_id();
    const int w = uniform((int)(threadIdx.x >> 6));
    if (threadIdx.x < 3 * NS) ctl[threadIdx.x] = (int)threadIdx.x >= 2 * NS ? -2 : 0;
    if (DICT) {
        for (int i = threadIdx.x; i < dict_bpw; i += blockDim.x) lbp[i] = dict_bp[i];
        for (int i = threadIdx.x; i < 8 * dict_NB; i += blockDim.x) lbt[i] = dict_bt[i];
        int32_t *lo = reinterpret_cast<int32_t *>(lbt + 8 * dict_NB);
        for (int i = threadIdx.x; i < dict_P * 8; i += blockDim.x) lo[i] = dict_off[i];
    }
    __syncthreads();
    // pattern id of v in [0, V): block id, then the block tuple's byte
    auto blk_of = [&](int v) -> uint32_t { return (lbp[v >> 7] >> (8 * ((v >> 5) & 3))) & 0xFFu; };
    auto pat_in = [&](uint32_t b, int v) -> uint32_t {
        return (lbt[b * 8 + ((v & 31) >> 2)] >> (8 * (v & 3))) & 0xFFu;
    };
    auto pat_of = [&](int v) -> uint32_t { return pat_in(blk_of(v), v); };

    if (w < NS) {
        // ------------------------------------------------------ a search wave
        if (flags & kFlagPrio) __builtin_amdgcn_s_setprio(3);
        const int pos = lane % LPR;
        const int sub = lane / LPR;
        const uint64_t lowmask = (LPR == 64) ? ~0ull : ((1ull << LPR) - 1ull);
        uint32_t *vis = lds + w * per;
        RT *ring = reinterpret_cast<RT *>(vis + VWp);   // (v[, depth])
        uint2 *q = qrec + w * kSplitQ;
        uint32_t *qd = qdep + w * kSplitQ;
        const int slot_id = blockIdx.x * NS + w;
        RT *spill = reinterpret_cast<RT *>(spill_all) + (size_t)slot_id * (size_t)V;
        int pub = 0, cons = 0;
#ifdef SDNR_STAMPS
        unsigned long long z_t0, z_t1, z_a, z_b, z_c, z_rd = 0, z_qw = 0, z_push = 0, z_it = 0,
                                                   z_nl = 0, z_sp = 0, z_rf = 0, z_rfc = 0;
        SDNR_STAMP(z_t0);
#endif
        // source order: blockIdx-strided, or (kFlagCuMap) the CU's own chunk
        const bool cumap = (flags & kFlagCuMap) != 0;
        int chunk = cumap ? split_cu_number(wq, nch, lane, err) : 0;
        auto next_source = [&](int prev) -> int {
            if (!cumap) return prev < 0 ? slot_id : prev + (int)gridDim.x * NS;
            return split_next_source(wq, nch, nsrc, &chunk, lane);
        };
        for (int si = next_source(-1); si < nsrc; si = next_source(si)) {
            const int s = uniform(src[si]);
            int32_t *prow = out_parent + (size_t)si * V;
            int32_t *trow = PACKED ? nullptr : out_port + (size_t)si * V;
            const size_t hb = (size_t)si * V;        // row of the hop table
            if (s < 0 || s >= V) {                 // unknown source: empty row
                for (int v = lane; v < V; v += SDNR_WAVE) {
                    prow[v] = -1;                  // packed: 0xFFFFFFFF
                    if (!PACKED) trow[v] = -1;
                    if (HOPS) put_hop(out_hops, hb + v, -1, flags);
                }
                continue;
            }
            for (int i = lane; i < VWp; i += SDNR_WAVE) vis[i] = 0u;
            if (lane == 0) {                       // the wave's LDS ops stay in order
                vis[vsw(s >> 5)] = 1u << (s & 31);
                prow[s] = PK == kTreePort16 ? (int32_t)((uint32_t)s | 0xFFFF0000u)
                        : PK == kTreeSlot  ? (int32_t)((uint32_t)s | (63u << 26)) : s;
                if (!PACKED) trow[s] = -1;
                if (HOPS) put_hop(out_hops, hb + s, 0, flags);
                ring[0] = RE::put((uint32_t)s, DICT ? pat_of(s) : 0u);
                __hip_atomic_store(&ctl[2 * NS + w], si, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            int lsp = 1, bot = 0, gsp = 0;
            int pubd = pub;                        // records announced to the writer
            for (;;) {
                if (lsp == 0) {
                    if (gsp == 0) break;
                    const int n = gsp < RING / 2 ? gsp : RING / 2;
                    // own spill stores: this wave wrote them through this
                    // CU's L1, so a workgroup-scope acquire (wait for them;
                    // no L1 invalidate) suffices -- the agent-scope one cost
                    // ~9.7 k cycles per refill under the writers' store
                    // traffic (stamps)
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    bot = (bot - n) & (RING - 1);
#ifdef SDNR_STAMPS
                    SDNR_STAMP(z_a);
#endif
                    for (int i = lane; i < n; i += SDNR_WAVE)
                        ring[(bot + i) & (RING - 1)] = spill[gsp - n + i];
                    gsp -= n;
                    lsp = n;
#ifdef SDNR_STAMPS
                    SDNR_STAMP(z_b);
                    z_rf++;
                    z_rfc += z_b - z_a;
#endif
                }
#ifdef SDNR_STAMPS
                SDNR_STAMP(z_a);
                z_it++;
#endif
                const int kk = lsp < K ? lsp : K;
                // every lane reads its slot's stack entry itself (no
                // cross-lane shuffle on the chain); slots past the stack
                // become vertex 0 and are masked below
                // (one slot per lane group: J == 1; with several groups per
                // lane, one read per lane + shuffles moves fewer LDS bytes)
                uint2 ue[J];
                int x[J];
                if (J == 1) {
                    ue[0] = RE::get(ring[(bot + lsp - 1 - sub) & (RING - 1)]);
                    ue[0].x = sub < kk ? ue[0].x : 0u;
                    if (DICT) ue[0].y = sub < kk ? ue[0].y : 0u;
                } else {
                    uint2 me = RE::get(ring[(bot + lsp - 1 - lane) & (RING - 1)]);
                    me.x = lane < kk ? me.x : 0u;
                    if (DICT) me.y = lane < kk ? me.y : 0u;
#pragma unroll
                    for (int j = 0; j < J; ++j) {
                        ue[j].x = (uint32_t)__shfl((int)me.x, j * R + sub);
                        ue[j].y = YR ? (uint32_t)__shfl((int)me.y, j * R + sub) : 0u;
                    }
                }
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    if constexpr (DICT) {
                        const int xj = (int)ue[j].x + loff[(int)(ue[j].y & 0xFFu) * 8 + pos];
                        x[j] = xj < V ? xj : -1;                 // padding: u + kDictPad
                    } else {
                        x[j] = split_row<FMT>(rows, rhi, V, W, (int)ue[j].x, pos);
                    }
                }
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const int ok = -(int)(((j * R + sub) < kk) & (pos < W));
                    x[j] = (x[j] & ok) | ~ok;
                }
                uint64_t m[J];
                uint32_t pw[J];                    // DICT: the pattern id of x[j]
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const int xi = x[j] & 0x7FFFFFFF;
                    const int xs = xi & ((x[j] >> 31) ^ -1);    // padding -> vertex 0
                    const uint32_t wv = vis[vsw(xs >> 5)];
                    // the block id beside the visited word, its tuple byte
                    // right behind (both off the ballot's path: only a push
                    // uses them)
                    if (DICT) pw[j] = pat_in(blk_of(xs), xs);
                    m[j] = __ballot((x[j] >= 0) & (((wv >> (xi & 31)) & 1u) == 0u));
                }
                // announce the previous push's records now: the LDS reads of
                // this batch have already waited for those writes, so the
                // LDS-only release costs no extra round trip
                if (pub != pubd) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                    if (lane == 0) __hip_atomic_store(&ctl[w], pub, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_WORKGROUP);
                    pubd = pub;
                }
                int jstar = J;
#pragma unroll
                for (int j = J - 1; j >= 0; --j)
                    if (m[j] != 0) jstar = j;
#ifdef SDNR_STAMPS
                SDNR_STAMP(z_b);
                z_rd += z_b - z_a;
#endif
                if (jstar == J) {
                    lsp -= kk;
                    continue;
                }
                uint64_t mj = 0;
                int vv = -1;
                uint32_t pv = 0;
                uint2 uj = make_uint2(0u, 0u);
#pragma unroll
                for (int j = 0; j < J; ++j)
                    if (j == jstar) {
                        mj = m[j];
                        vv = x[j];
                        if (DICT) pv = pw[j];
                        uj = ue[j];
                    }
                const int sstar = (__ffsll((unsigned long long)mj) - 1) / LPR;
                const int istar = jstar * R + sstar;
                const uint64_t mm = mj & (lowmask << (sstar * LPR));
                const int eu = read_lane((int)uj.x, sstar * LPR);
                const uint32_t ey = YR ? (uint32_t)read_lane((int)uj.y, sstar * LPR) : 0u;
                const uint32_t ed = DICT ? ey >> 8 : ey;   // the popped entry's depth
                lsp -= istar + 1;
                const int cnt = __popcll(mm);
                // room in the record queue (the writer publishes its progress)
                if (pub + cnt - cons > kSplitQ) {
                    if (pub != pubd) {             // the writer must see what is queued
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                        if (lane == 0) __hip_atomic_store(&ctl[w], pub, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_WORKGROUP);
                        pubd = pub;
                    }
                    for (unsigned spin = 0; pub + cnt - cons > kSplitQ; ++spin) {
                        cons = __hip_atomic_load(&ctl[NS + w], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (pub + cnt - cons <= kSplitQ) break;
                        if (spin > kSpin) {
                            if (lane == 0) atomicOr(err, 4);
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
#ifdef SDNR_STAMPS
                SDNR_STAMP(z_c);
                z_qw += z_c - z_b;
                z_nl++;
                if (lsp + cnt > RING) z_sp++;
#endif
                if (lsp + cnt > RING) {            // spill the oldest half
                    for (int i = lane; i < RING / 2; i += SDNR_WAVE)
                        spill[gsp + i] = ring[(bot + i) & (RING - 1)];
                    gsp += RING / 2;
                    bot = (bot + RING / 2) & (RING - 1);
                    lsp -= RING / 2;
                }
                if ((mm >> lane) & 1ull) {
                    const int rank = lanes_below(mm);
                    atomicOr(&vis[vsw(vv >> 5)], 1u << (vv & 31));
                    q[(pub + rank) & (kSplitQ - 1)] =
                        make_uint2((uint32_t)vv | ((uint32_t)pos << 26), (uint32_t)eu);
                    if (HOPS) qd[(pub + rank) & (kSplitQ - 1)] = ed + 1u;
                    ring[(bot + lsp + rank) & (RING - 1)] =
                        RE::put((uint32_t)vv, DICT ? pv | ((ed + 1u) << 8) : ed + 1u);
                }
                lsp += cnt;
                pub += cnt;
#ifdef SDNR_STAMPS
                SDNR_STAMP(z_a);
                z_push += z_a - z_c;
#endif
            }
            if (pub != pubd) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                if (lane == 0) __hip_atomic_store(&ctl[w], pub, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            // this source's records drained before its row changes, then the
            // entries of unreached vertices
            for (unsigned spin = 0; cons != pub; ++spin) {
                cons = __hip_atomic_load(&ctl[NS + w], __ATOMIC_ACQUIRE,
                                         __HIP_MEMORY_SCOPE_WORKGROUP);
                if (cons == pub) break;
                if (spin > kSpin) {
                    if (lane == 0) atomicOr(err, 8);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            for (int v = lane; v < V; v += SDNR_WAVE) {
                if (((vis[vsw(v >> 5)] >> (v & 31)) & 1u) == 0u) {
                    prow[v] = -1;
                    if (!PACKED) trow[v] = -1;
                    if (HOPS) put_hop(out_hops, hb + v, -1, flags);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        if (lane == 0) __hip_atomic_store(&ctl[2 * NS + w], -1, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_WORKGROUP);
#ifdef SDNR_STAMPS
        SDNR_STAMP(z_t1);
        if (lane == 0) {
            atomicAdd(&g_stamp[0], z_t1 - z_t0);   // search wave lifetime
            atomicAdd(&g_stamp[1], z_rd);          // stack + row + visited per iteration
            atomicAdd(&g_stamp[2], z_it);          // iterations
            atomicAdd(&g_stamp[3], z_nl);          // non-leaf pops
            atomicAdd(&g_stamp[4], z_qw);          // queue-room waits
            atomicAdd(&g_stamp[5], z_push);        // push (+ spill)
            atomicAdd(&g_stamp[6], z_sp);          // spills
            atomicAdd(&g_stamp[7], z_rf);          // refills
            atomicAdd(&g_stamp[8], z_rfc);         // refill cycles
        }
#endif
    } else {
        split_writer<NS, HOPS, PK>(V, W, ell_port, qrec, qdep, ctl, lane, out_parent, out_port,
                                   out_hops, err, flags);
    }
}

// ---------------------------------------------------------------------------
// Asynchronous counted pops (the k=48 headline kernel).
//
// Same counts as dfs_count_kernel, one observation further: a count may be
// STALE HIGH without breaking exactness.  If the skip stops at an entry whose
// count still includes a neighbour visited a moment ago, the row check finds
// no fresh child and the entry is popped as the leaf pop it is.  A count is
// never low (a decrement is published only after its mark).  So the
// decrements need not finish before the next pop: wave 0 runs the search
// chain alone -- skip, row, visited gather, push -- with no barrier, and
// publishes each push's children into an LDS ring; waves 1..NW-1 drain the
// ring (child j belongs to worker 1 + j % (NW-1)), load the children's
// in-rows and ds_sub the counts.  Hand-off inside the workgroup: ring writes,
// release fence, relaxed store of the published count; workers acquire-load
// it.  Back-pressure keeps the ring from overrunning the slowest worker.
// Every spin is bounded; the bound only trips on a bug, and then sets the
// error word instead of hanging the GPU.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int swz(int x) { return lds_swz(x); }   // common.h

// the parts of the quotient's flush ("The quotient's flush";
// A/B builds: -DSDNR_QUOT_FLUSH=n leaves some out, 0 keeps the four dependent
// trips per vertex): 1 a tree link's port comes from the composed table
// (sdnr_quot::qport; the root's children take their slot there and the port
// from the root's own row, kept in LDS), 2 the workers record every pushed
// class's offset into the slot table.  (A third part, the vertices' classes
// loaded before the barrier that ends the search, gained nothing at the
// headline and cost the 1,152-live row 2 us: profiles/quot_flush_ab.txt)
#ifndef SDNR_QUOT_FLUSH
#define SDNR_QUOT_FLUSH 3
#endif

// the quotient's tables come through pointers read from device memory
// (sdnr_quot), which the compiler takes for generic ones: flat loads, counted
// as LDS operations too, so every LDS wait would wait for them.  They are global
template <class T> using gptr = const __attribute__((address_space(1))) T *;
template <class T> __device__ __forceinline__ gptr<T> as_global(const T *p) { return (gptr<T>)p; }

// PAIR: how a worker loads the pre-swizzled in-rows -- 0: one u16 row (64
// lanes) per child; 1: rows of <= 32 entries repeated in lanes 32..63, one
// load for two children; 2: the 64-entry rows read as 32 u32 words, lanes
// 0..31 child 2g and 32..63 child 2g + 1, two ds_sub per lane -- half the
// load instructions and half the returned dwords of PAIR 0 (the CU's
// vector-memory data return is 71 % busy at the k=48 headline's load)
// SPEC: the speculative stack pop (kFlagSpecPop) compiled in.  A separate
// instantiation, not only a runtime flag: its code in the hot loop costs the
// low-load (<= 2 sources per CU) kernel ~8 us at k=48 even when the flag is
// off (144 sources 44.3 vs 52.0 us, same box, gpurun_out/r5_abr4), while at
// the headline's load the pop itself gains
template <int NW, bool HOPS, bool PACKED, bool C16, int PAIR, bool SPEC = false, bool QUOT = false>
__global__ __launch_bounds__(NW * 64, C16 ? 7 : 1) void dfs_async_kernel(
    int V, const uint16_t *__restrict__ adj, const uint16_t *__restrict__ radj,
    const uint32_t *__restrict__ deg, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ port, int W, const int32_t *__restrict__ ell_port,
    const int32_t *__restrict__ src, int nsrc, int32_t *__restrict__ out_parent,
    int32_t *__restrict__ out_port, int32_t *__restrict__ out_hops, int *__restrict__ err,
    int flags, const int32_t *__restrict__ live,
    // QUOT, the twin-class quotient: V, adj, radj and deg
    // are the quotient's, qt->VR the graph's vertex count -- the length of a
    // table row --, and the tables are expanded in the flush: cid[v] = class
    // | rank << 16, info[c] = largest member | twins << 16, slot[loff[c * 64
    // + slot] + rank] the tree link's slot in the real row, qport[the same
    // index] its port.  A separate
    // instantiation: as a runtime branch its pointers cost every form
    // registers (scalar spills 5 -> 32, the plain 4-wave forms 6 -> 5 waves
    // per SIMD by the compiler's resource remarks), the graph's own search
    // among them; one pointer, so the search loop carries two more scalars
    const sdnr_quot *__restrict__ qt)
{
    static_assert(NW >= 2, "wave 0 searches, the others decrement");
    constexpr bool quot = QUOT;
    const int VT = quot ? uniform((int)qt->VR) : V;   // entries of a table row
    // the twin fold's live count (device memory: the host does not know it):
    // only src[0 .. *live) is searched, no row is written behind it
    if (live) nsrc = min(nsrc, *live);
    constexpr int U = 4;                         // init / flush vertices per thread per step
    constexpr int S = NW - 1;                    // workers
    constexpr int RING = 512;                    // children in flight (u16)
#ifndef SDNR_ASYNC_G
#define SDNR_ASYNC_G 8
#endif
// table flush: vertices per thread per pass (one pass for k=48's 2,880
// switches at 8 waves: 1 / 144 sources 45.4 / 47.1 -> 43.7 / 45.1 us; 12
// gained 1 % more there but cost the dragonfly's compact kernel registers:
// 2,064 sources 169 -> 217 us; profiles/r06_flush_ab)
#ifndef SDNR_ASYNC_FLUSH_U
#define SDNR_ASYNC_FLUSH_U 6
#endif
#ifndef SDNR_ASYNC_G_DW
#define SDNR_ASYNC_G_DW 16
#endif
#ifndef SDNR_ASYNC_G_P1
#define SDNR_ASYNC_G_P1 8
#endif
#ifndef SDNR_ASYNC_G_U16
#define SDNR_ASYNC_G_U16 48
#endif
// the dword-paired rows at 4 waves: the folded search's low-load form only
// (dfs_dispatch).  48 live searches of 1,152 sources, us per call at 8 / 16 /
// 32 / 48: 86.3 / 72.4 / 64.1 / 64.4, the u16 rows 67.3
#ifndef SDNR_ASYNC_G_DW4
#define SDNR_ASYNC_G_DW4 32
#endif
    // children per worker step: 16 (8 above 4 waves), and 16 with the
    // dword-paired rows of the 5-worker regime (8 loads): k=48 144 sources
    // 54.9 -> 48.8 us, one source 53.3 -> 47.2 us (fresher counts)
    // Round 5: 32 with the plain u16 in-rows at <= 4 waves (the k=48
    // headline; library A/B, one box, gpurun_out/r5_abg3: 1,152 sources
    // 82.5 / 80.6 / 79.4 / 78.8 / 85.1 us at 16 / 24 / 32 / 48 / 64, 576
    // sources 67.4 -> 64.9 at 32), while the dragonfly's paired rows want
    // narrower steps: 8 (2,064 sources 178.9 / 171.8 / 168.5 us at 16 / 12 /
    // 8, 214.1 at 32; gpurun_out/r5_abg5).  48 for the plain rows after a
    // second A/B on the final library (profiles/r05_async_g48_ab.log): 1,152
    // sources 79.5 -> 78.2 us, every smaller share within 0.3 us
    constexpr int G = NW <= 4 ? (PAIR == 0 ? SDNR_ASYNC_G_U16
                                           : (PAIR == 2 && NW == 4 ? SDNR_ASYNC_G_DW4 : SDNR_ASYNC_G))
                              : (PAIR == 2 ? SDNR_ASYNC_G_DW : (PAIR == 1 ? SDNR_ASYNC_G_P1 : 8));
    constexpr unsigned kSpin = 1u << 22;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int VW = (V + 1 + 31) >> 5;
    const int VWp = (VW + 3) & ~3;
    // C16 (compact): u16 counts in pairs, u16 parents + u8 slots -- 2,064
    // dragonfly sources fit 9 per CU (all resident) instead of 6
    // count words, swizzled within 32-word groups, then 64 dummy words (the
    // pre-swizzled in-rows' padding targets, one per lane), whole 256-blocks
    const int CWp = ((((C16 ? (V + 2) >> 1 : V + 1) + 31) & ~31) + 64 + 255) & ~255;
    const int SWp = (((V + 1) >> 1) + 3) & ~3;
    const int PW = (V + 255) & ~255;                         // parent entries
    const int PWp = C16 ? PW / 2 + PW / 4 : PW;
    uint32_t *vis = lds;
    uint32_t *cnt = vis + VWp;                   // cnt[swz(v)] (C16: swz(v >> 1), halves)
    uint16_t *stk = reinterpret_cast<uint16_t *>(cnt + CWp);
    uint32_t *ps = cnt + CWp + SWp;              // ps[swz(v)] = parent | slot << 16
    uint16_t *ps16 = reinterpret_cast<uint16_t *>(ps);        // C16: ps16[swz(v)] = parent
    uint8_t *sl8 = reinterpret_cast<uint8_t *>(ps16 + PW);    //      sl8[swz(v)] = slot
    uint16_t *dep = reinterpret_cast<uint16_t *>(ps + PWp);   // dep[v]
    auto cnt_of = [&](int v) -> uint32_t {
        if constexpr (C16) {
            const uint32_t x = __hip_atomic_load(&cnt[swz(v >> 1)], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
            return (x >> ((v & 1) << 4)) & 0xFFFFu;
        } else {
            return __hip_atomic_load(&cnt[swz(v)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    uint16_t *ring = reinterpret_cast<uint16_t *>(ps + PWp + (HOPS ? ((V + 1) >> 1) : 0));
    int *ctl = reinterpret_cast<int *>(ring + RING);   // [0] published [1] done [2+k] consumed
    // QUOT: qlo[c] = the slot-table offset of the link class c was pushed
    // over, written by the worker that drains c from the ring and used by the
    // flush where vis[c] is set and nowhere else (a word of an earlier source
    // is never used: every marked class but the root's own went through the
    // ring); rport = the port row of the source itself (its children's ports)
    constexpr bool qf_port = quot && (SDNR_QUOT_FLUSH & 1), qf_rec = quot && (SDNR_QUOT_FLUSH & 2);
    uint32_t *qlo = reinterpret_cast<uint32_t *>(ctl + 16);
    int32_t *rport = reinterpret_cast<int32_t *>(qlo + ((V + 3) & ~3));
    const int lane = lane_id();
    const int w = uniform((int)(threadIdx.x >> 6));
#ifdef SDNR_STAMPS
    unsigned long long kstart;
    SDNR_STAMP(kstart);
#endif

    for (int si = blockIdx.x; si < nsrc; si += gridDim.x) {
        const int sr = uniform(src[si]);         // the source as the caller names it
        int32_t *prow = out_parent + (size_t)si * VT;
        int32_t *trow = PACKED ? nullptr : out_port + (size_t)si * VT;
        const size_t hb = (size_t)si * VT;       // row of the hop table
        if (sr < 0 || sr >= VT) {
            for (int v = threadIdx.x; v < VT; v += blockDim.x) {
                prow[v] = -1;                    // packed: 0xFFFFFFFF
                if (!PACKED) trow[v] = -1;
                if (HOPS) put_hop(out_hops, hb + v, -1, flags);
            }
            continue;
        }
        // the vertex searched from: the source, or its class in the quotient.
        // A class of several members is explored first but not marked: the
        // other members are pushed by whoever has the class in their row
        int s = sr;
        bool rootvis = true;
        if constexpr (quot) {
            s = uniform((int)(qt->cid[sr] & 0xFFFFu));
            rootvis = uniform((int)(qt->info[s] >> 16)) == 0;
        }
#ifdef SDNR_STAMPS
        unsigned long long ph0, ph1, ph2, ph3;
        SDNR_STAMP(ph0);
#endif
        // the source's own port row, beside the counts' loads (both port
        // arrays carry a wave of padding behind the last row)
        int rp0 = -1;
        if constexpr (qf_port) {
            if (w == NW - 1)
                rp0 = W > 0 ? ell_port[(size_t)sr * W + lane] : port[row_ptr[sr] + lane];
        }
        for (int i = threadIdx.x; i < VW; i += blockDim.x) vis[i] = 0u;
        // counts start at the out-degrees: U independent loads per thread in
        // flight before the LDS stores
        if constexpr (C16) {                     // deg is padded to an even length
            const int nw = (V + 2) >> 1;
            for (int i0 = threadIdx.x; i0 < nw; i0 += U * blockDim.x) {
                uint2 dg[U];
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const int i = i0 + k * (int)blockDim.x;
                    dg[k] = reinterpret_cast<const uint2 *>(deg)[i < nw ? i : 0];
                }
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const int i = i0 + k * (int)blockDim.x;
                    if (i < nw) cnt[swz(i)] = dg[k].x | (dg[k].y << 16);
                }
            }
        } else {
            for (int i0 = threadIdx.x; i0 <= V; i0 += U * blockDim.x) {
                uint32_t dg[U];
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const int i = i0 + k * (int)blockDim.x;
                    dg[k] = deg[i <= V ? i : V];
                }
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const int i = i0 + k * (int)blockDim.x;
                    if (i <= V) cnt[swz(i)] = dg[k];
                }
            }
        }
        if (threadIdx.x < 2 + S) ctl[threadIdx.x] = 0;
        if constexpr (qf_port) {
            if (w == NW - 1) rport[lane] = rp0;
        }
        __syncthreads();
#ifdef SDNR_STAMPS
        SDNR_STAMP(ph1);
#endif

        if (w == 0) {
            // ------------------------------------------------ the search
            if (flags & kFlagPrio) __builtin_amdgcn_s_setprio(3);
            const int pub0 = rootvis ? 1 : 0;
            if (lane == 0) {
                if (rootvis) vis[s >> 5] |= 1u << (s & 31);
                vis[V >> 5] |= 1u << (V & 31);
                if (C16) ps16[swz(s)] = (uint16_t)s;
                else ps[swz(s)] = (uint32_t)s;
                if (HOPS) dep[s] = 0;
                stk[0] = (uint16_t)s;
                ring[0] = (uint16_t)s;           // s's in-neighbours lose one (rootvis)
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) __hip_atomic_store(&ctl[0], pub0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            int pub = pub0, pubd = pub0, sp = 1, lo = 0; // published / announced
            constexpr int NPF = 1;        // rows of the NPF largest children in flight
            // the prefetched rows stay u16 across the loop back-edge: an int
            // copy there needs the load's data (s_waitcnt vmcnt(0) at the end
            // of every push), a u16 one is widened where the row is used
            int pu[NPF];
            uint16_t xp[NPF];
#pragma unroll
            for (int k = 0; k < NPF; ++k) {
                pu[k] = -1;
                xp[k] = (uint16_t)V;
            }
#ifdef SDNR_STAMPS
            unsigned long long st_t0, st_t1, st_row = 0, st_cand = 0, st_false = 0, st_bp = 0,
                                               st_miss = 0, st_skip = 0, st_tc = 0, st_skipc = 0,
                                               st_pushc = 0;
            SDNR_STAMP(st_t0);
            st_tc = st_t0;
#endif
            // one candidate: its row, fresh children, push; returns the
            // next candidate when it is one of the new children (the
            // common case: a tight inner loop), else -1 (pop from the stack)
            auto explore = [&](const int u) -> int {
#ifdef SDNR_STAMPS
                unsigned long long ta, tb;
                SDNR_STAMP(ta);
                st_skipc += ta - st_tc;
                {
                    bool hit = false;
#pragma unroll
                    for (int k = 0; k < NPF; ++k) hit |= u == pu[k];
                    if (!hit) st_miss++;
                }
#endif
                int x = -1;
#pragma unroll
                for (int k = 0; k < NPF; ++k)
                    if (x < 0 && u == pu[k]) x = (int)xp[k];
                if (x < 0) x = (int)adj[(size_t)u * 64 + lane];
                const uint32_t wv = vis[x >> 5];
                // the row's counts ride along with its visited words (one
                // wait for both; read in every lane: x <= V is always a count
                // word); a count read earlier is at most staler, i.e. high,
                // which the row check absorbs -- so a plain load will do (as
                // an atomic load it waited for this wave's earlier LDS writes)
                uint32_t cc;
                if constexpr (C16)
                    cc = (cnt[swz(x >> 1)] >> ((x & 1) << 4)) & 0xFFFFu;
                else
                    cc = cnt[swz(x)];
                const bool fresh = ((wv >> (x & 31)) & 1u) == 0u;
                const uint64_t mm = __ballot(fresh);
                // balloted here, ahead of the leaf-pop exit, so the count
                // read stays beside the visited read (used after the exit, the
                // compiler sank it there: a second round trip)
                const uint64_t ccm = __ballot(cc != 0u);
#ifdef SDNR_STAMPS
                SDNR_STAMP(tb);
                st_row += tb - ta;
                st_cand++;
                if (mm == 0) st_false++;
#endif
#ifdef SDNR_STAMPS
                if (mm == 0) st_tc = tb;
#endif
                if (mm == 0) return -1;          // stale count: a leaf pop after all
                const int c = __popcll(mm);
                const int rank = lanes_below(mm);
                // the next candidate is known here, the counts having come
                // with the visited words: the highest fresh child with a count
                // (the children above it are leaves -- counts are never low --
                // and are popped).  Its row is the one prefetched, and its
                // stack position is a scalar popcount: one ballot -> readlane
                // chain per candidate instead of two
                const uint64_t mc = ccm & mm;
                int nu = -1, below = 0;
                if (mc) {
                    const int hl = highest_lane(mc);
                    nu = read_lane(x, hl);
                    below = __popcll(mm & ((1ull << hl) - 1ull));   // fresh children under it
                    pu[0] = nu;
                    xp[0] = adj[(size_t)nu * 64 + lane];
                } else if (SPEC && (flags & kFlagSpecPop) && sp > 0) {
                    // every fresh child is a leaf (its count is 0 and counts
                    // never rise), so none stays on the stack and the next
                    // candidate is the first entry with a count from the top
                    // of the stack as it is NOW: the push below writes only
                    // above sp and changes no count.  Its window, counts and
                    // row are read here, so the row load runs beside the
                    // push (a count read early is at most staler -- high --
                    // which the row check absorbs).  A window without a
                    // candidate is skipped as the outer loop would.
                    const int kk = sp < 64 ? sp : 64;
                    const int at = sp - 1 - lane;
                    int e2 = stk[at < 0 ? 0 : at];
                    e2 = lane < kk ? e2 : V;
                    uint32_t c2;
                    if constexpr (C16)
                        c2 = (cnt[swz(e2 >> 1)] >> ((e2 & 1) << 4)) & 0xFFFFu;
                    else
                        c2 = cnt[swz(e2)];
                    const uint64_t m2 = __ballot(c2 != 0u);
                    if (m2) {
                        const int f2 = __ffsll((unsigned long long)m2) - 1;
                        nu = read_lane(e2, f2);
                        sp -= f2 + 1;
                        pu[0] = nu;
                        xp[0] = adj[(size_t)nu * 64 + lane];
                    } else {
                        sp -= kk;
                        pu[0] = -1;
                    }
                } else {
                    pu[0] = -1;                  // the next candidate comes off the stack
                }
                int du = 0;
                if (HOPS) du = uniform((int)dep[u]);
                // back-pressure: ring slots below every worker's progress are
                // free; the bound only needs refreshing when it would block
                for (unsigned spin = 0; pub + c - lo > RING; ++spin) {
                    lo = 0x7FFFFFFF;
#pragma unroll
                    for (int q = 0; q < S; ++q)
                        lo = min(lo, __hip_atomic_load(&ctl[2 + q], __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_WORKGROUP));
                    lo = uniform(lo);            // scalar: the bound test stays off the VALU
                    if (pub + c - lo <= RING) break;
                    if (spin > kSpin) {
                        if (lane == 0) atomicOr(err, 1);
                        break;
                    }
#ifdef SDNR_STAMPS
                    st_bp++;
#endif
                    __builtin_amdgcn_s_sleep(1);
                }
                if (fresh) {
                    atomicOr(&vis[x >> 5], 1u << (x & 31));
                    if (C16) {
                        ps16[swz(x)] = (uint16_t)u;
                        sl8[swz(x)] = (uint8_t)lane;
                    } else {
                        ps[swz(x)] = (uint32_t)u | ((uint32_t)lane << 16);
                    }
                    if (HOPS) dep[x] = (uint16_t)(du + 1);
                    stk[sp + rank] = (uint16_t)x;
                    ring[(pub + rank) & (RING - 1)] = (uint16_t)x;
                }
                pub += c;
                // announce the children without waiting for the writes: one
                // wave's LDS ops execute in issue order, so a worker that
                // reads the new count reads the ring after its entries were
                // written; the empty asm keeps the compiler from moving the
                // store above them
                __asm__ volatile("" ::: "memory");
                if (lane == 0) __hip_atomic_store(&ctl[0], pub, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_WORKGROUP);
                pubd = pub;
                sp += below;
#ifdef SDNR_STAMPS
                SDNR_STAMP(st_tc);
                st_pushc += st_tc - tb;
#endif
                return nu;
            };
            for (;;) {
                uint64_t m = 0;
                int e = V;
                while (sp > 0) {
#ifdef SDNR_STAMPS
                    st_skip++;
#endif
                    const int kk = sp < 64 ? sp : 64;
                    const int at = sp - 1 - lane;
                    e = stk[at < 0 ? 0 : at];
                    e = lane < kk ? e : V;
                    const uint32_t c = cnt_of(e);
                    m = __ballot(c != 0u);
                    if (m) break;
                    sp -= kk;
                }
                // children of the last push not yet announced (the push
                // block announces its own; kept for the first pops)
                if (pub != pubd) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                    if (lane == 0) __hip_atomic_store(&ctl[0], pub, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_WORKGROUP);
                    pubd = pub;
                }
                if (!m) break;
                const int first = __ffsll((unsigned long long)m) - 1;
                sp -= first + 1;
                for (int u = read_lane(e, first); u >= 0;) u = explore(u);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) __hip_atomic_store(&ctl[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (flags & kFlagPrio) __builtin_amdgcn_s_setprio(0);
#ifdef SDNR_STAMPS
            SDNR_STAMP(st_t1);
            if (lane == 0) {
                atomicAdd(&g_stamp[0], st_t1 - st_t0);   // search wave lifetime
                atomicAdd(&g_stamp[1], st_row);          // row + gather cycles
                atomicAdd(&g_stamp[2], st_cand);         // candidates popped
                atomicAdd(&g_stamp[3], st_false);        // ... with no fresh child
                atomicAdd(&g_stamp[4], st_bp);           // back-pressure sleeps
                atomicAdd(&g_stamp[5], st_skip * 1000000ull + st_miss);   // skips, prefetch misses
                atomicAdd(&g_stamp[6], st_skipc);        // skip cycles
                atomicAdd(&g_stamp[7], st_pushc);        // push+publish cycles
            }
#endif
        } else {
            // ------------------------------------------------ the decrements
            int j = w - 1;                       // next child index of this worker
            gptr<uint32_t> wloff = nullptr;
            if constexpr (qf_rec) wloff = as_global(qt->loff);
            for (unsigned spin = 0;;) {
                const int P = __hip_atomic_load(&ctl[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (j >= P) {
                    if (__hip_atomic_load(&ctl[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) &&
                        j >= __hip_atomic_load(&ctl[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP))
                        break;
                    if (++spin > kSpin) {
                        if (lane == 0) atomicOr(err, 2);
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                spin = 0;
                const int n = (P - j + S - 1) / S < G ? (P - j + S - 1) / S : G;
                const int mine = lane < n ? (int)ring[(j + lane * S) & (RING - 1)] : V;
                // QUOT: the class's record is final at its push (the search
                // wave wrote it before the ring entry), so the slot-table
                // offset of its tree link is loaded here, off the search's
                // chain, beside the in-rows, and kept for the flush; the root's
                // own entry (index 0 of a marked root) has no link
                uint32_t qo = 0u;
                bool qrec = false;
                if constexpr (qf_rec) {
                    qrec = lane < n && (j + lane * S > 0 || !rootvis);
                    if (qrec) {
                        uint32_t xx;
                        if (C16) xx = (uint32_t)ps16[swz(mine)] | ((uint32_t)sl8[swz(mine)] << 16);
                        else xx = ps[swz(mine)];
                        qo = wloff[(size_t)(xx & 0xFFFFu) * 64 + (xx >> 16)];
                    }
                }
                if constexpr (PAIR == 2) {
                    constexpr int G2 = G / 2;
                    const int hiw = lane >> 5;
                    const uint32_t *rw32 = reinterpret_cast<const uint32_t *>(radj);
                    uint32_t r[G2];
#pragma unroll
                    for (int g = 0; g < G2; ++g) {
                        const int ca = read_lane(mine, 2 * g), cb = read_lane(mine, 2 * g + 1);
                        r[g] = rw32[(size_t)(hiw ? cb : ca) * 32 + (lane & 31)];
                    }
#pragma unroll
                    for (int g = 0; g < G2; ++g)
                        if (2 * g + hiw < n) {
                            atomicSub(&cnt[r[g] & 0xFFFFu], 1u);
                            atomicSub(&cnt[r[g] >> 16], 1u);
                        }
                    if constexpr (qf_rec) {
                        if (qrec) qlo[mine] = qo;
                    }
                    j += n * S;
                    if (lane == 0) __hip_atomic_store(&ctl[2 + w - 1], j, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_WORKGROUP);
                    continue;
                }
                if constexpr (PAIR == 1) {
                    // rows repeat in lanes 32..63: load g serves child 2g in
                    // lanes 0..31 and child 2g + 1 in lanes 32..63 (a template
                    // case: a runtime branch here cost the unpaired k=48
                    // kernel 3 %)
                    constexpr int G2 = G / 2;
                    const int hiw = lane >> 5;
                    int r[G2];
#pragma unroll
                    for (int g = 0; g < G2; ++g) {
                        const int ca = read_lane(mine, 2 * g), cb = read_lane(mine, 2 * g + 1);
                        r[g] = radj[(size_t)(hiw ? cb : ca) * 64 + lane];
                    }
#pragma unroll
                    for (int g = 0; g < G2; ++g)
                        if (2 * g + hiw < n) {
                            if (C16) atomicSub(&cnt[r[g] >> 1], 1u << ((r[g] & 1) << 4));
                            else atomicSub(&cnt[r[g]], 1u);
                        }
                    if constexpr (qf_rec) {
                        if (qrec) qlo[mine] = qo;
                    }
                    j += n * S;
                    if (lane == 0) __hip_atomic_store(&ctl[2 + w - 1], j, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_WORKGROUP);
                    continue;
                }
                int r[G];
                // unconditional: a slot past n loads the sentinel row V (L2
                // resident); guarding each load measured 20 % slower
#pragma unroll
                for (int g = 0; g < G; ++g) r[g] = radj[(size_t)read_lane(mine, g) * 64 + lane];
                if (flags & kFlagPreSwz) {
                    // pre-swizzled in-rows: entries are count-word indices
                    // (C16: word << 1 | half), padding points at a dummy
                    // word of its lane past the counts -- no compare, mask
                    // or swizzle arithmetic per child
#pragma unroll
                    for (int g = 0; g < G; ++g)
                        if (g < n) {
                            if (C16) atomicSub(&cnt[r[g] >> 1], 1u << ((r[g] & 1) << 4));
                            else atomicSub(&cnt[r[g]], 1u);
                        }
                } else {
#pragma unroll
                    for (int g = 0; g < G; ++g)
                        if (g < n && r[g] != V) {
                            if (C16) atomicSub(&cnt[swz(r[g] >> 1)], 1u << ((r[g] & 1) << 4));
                            else atomicSub(&cnt[swz(r[g])], 1u);
                        }
                }
                if constexpr (qf_rec) {
                    if (qrec) qlo[mine] = qo;
                }
                j += n * S;
                if (lane == 0) __hip_atomic_store(&ctl[2 + w - 1], j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
#ifdef SDNR_STAMPS
        SDNR_STAMP(ph2);
#endif

        // tables: UF vertices per thread, their port loads (one ELL load, or
        // row_ptr + port) all in flight before the stores.  A wave's
        // vector-memory counter retires loads and stores in issue order, so
        // a port gather issued after the previous pass's table stores waits
        // for their acknowledgement: fewer, wider passes (k=48 at 8 waves:
        // one pass)
        constexpr int UF = SDNR_ASYNC_FLUSH_U;
        // the quotient's records expanded to the graph's vertices: v takes
        // the record of its class (the root marker for the source itself);
        // the real parent is the source where the pusher is the source's
        // class, else the pusher's largest member.  After the coalesced load
        // of v's class, the record and the offset the workers kept for it are
        // in LDS, so one stage of gathers is left: the real parent, and one
        // word at (offset + rank) -- the link's port from the composed table,
        // or for a child of the root the dword of the slot table that holds
        // its slot, the port then being the root's own (rport, LDS).  No
        // branch per vertex (a branch around a gather made it wait for the one
        // before): a vertex without a tree link gathers at index 0 of every
        // table and drops the result -- so does the word LDS holds for a
        // class without a mark, which may be an earlier source's.  All UF
        // vertices' gathers are in flight together, and all before the stores.
        // (SDNR_QUOT_FLUSH without its part 2 loads the offset in a stage of
        // its own, without its part 1 the slot and then the port from the
        // parent's row: the four dependent trips this replaced)
        if constexpr (quot) {
            const gptr<uint32_t> qcid = as_global(qt->cid), qinfo = as_global(qt->info),
                                 qloff = as_global(qt->loff);
            const gptr<uint8_t> qslot = as_global(qt->slot);
            const gptr<int32_t> qport = as_global(qt->qport);
            for (int v0 = threadIdx.x; v0 < VT; v0 += UF * blockDim.x) {
                uint32_t ck[UF], lf[UF], pi[UF], val[UF];
                int p[UF], pt[UF], hp[UF];
                bool ok[UF], rc[UF];             // a tree link; ... from the root
#pragma unroll
                for (int k = 0; k < UF; ++k) {
                    const int v = v0 + k * (int)blockDim.x;
                    ck[k] = qcid[v < VT ? v : 0];
                }
#pragma unroll
                for (int k = 0; k < UF; ++k) {
                    const int v = v0 + k * (int)blockDim.x;
                    const int c = (int)(ck[k] & 0xFFFFu);
                    const uint32_t vw = vis[c >> 5];
                    uint32_t xx;
                    if (C16) xx = (uint32_t)ps16[swz(c)] | ((uint32_t)sl8[swz(c)] << 16);
                    else xx = ps[swz(c)];
                    uint32_t off = 0u;
                    if (qf_rec) off = qlo[c];
                    int d = 0;
                    if (HOPS) d = (int)dep[c];
                    ok[k] = v < VT && v != sr && ((vw >> (c & 31)) & 1u);
                    const int pc = ok[k] ? (int)(xx & 0xFFFFu) : 0;
                    rc[k] = ok[k] && pc == s;
                    p[k] = pc;
                    if (qf_rec) lf[k] = ok[k] ? off + (ck[k] >> 16) : 0u;
                    else lf[k] = ok[k] ? (uint32_t)pc * 64u + (xx >> 16) : 0u;
                    hp[k] = ok[k] ? d : (v == sr ? 0 : -1);
                }
                if constexpr (!qf_rec) {
#pragma unroll
                    for (int k = 0; k < UF; ++k) pi[k] = qinfo[p[k]];
#pragma unroll
                    for (int k = 0; k < UF; ++k) {
                        const uint32_t o = qloff[lf[k]];
                        lf[k] = ok[k] ? o + (ck[k] >> 16) : 0u;
                    }
                }
#pragma unroll
                for (int k = 0; k < UF; ++k) {
                    if (qf_rec) pi[k] = qinfo[p[k]];
                    if (qf_port) {
                        const gptr<uint32_t> at =
                            rc[k] ? reinterpret_cast<gptr<uint32_t>>(qslot + (lf[k] & ~3u))
                                  : reinterpret_cast<gptr<uint32_t>>(qport + lf[k]);
                        val[k] = *at;
                    } else {
                        val[k] = (uint32_t)qslot[lf[k]];
                    }
                }
                // the gathered words are taken here, behind the last gather's
                // issue (left to the compiler, the first vertex's parent load
                // sank into the branch that uses it, behind a wait for all)
#pragma unroll
                for (int k = 0; k < UF; ++k) __asm__ volatile("" : "+v"(pi[k]), "+v"(val[k]));
#pragma unroll
                for (int k = 0; k < UF; ++k) {
                    const int v = v0 + k * (int)blockDim.x;
                    p[k] = ok[k] ? (rc[k] ? sr : (int)(pi[k] & 0xFFFFu)) : (v == sr ? sr : -1);
                    if (qf_port) {
                        const int own = rport[(val[k] >> ((lf[k] & 3u) << 3)) & 63u];
                        pt[k] = ok[k] ? (rc[k] ? own : (int)val[k]) : -1;
                    } else {
                        const int pp = ok[k] ? p[k] : 0;
                        pt[k] = W > 0 ? ell_port[(size_t)pp * W + val[k]]
                                      : port[row_ptr[pp] + (int)val[k]];
                        pt[k] = ok[k] ? pt[k] : -1;
                    }
                }
#pragma unroll
                for (int k = 0; k < UF; ++k) {
                    const int v = v0 + k * (int)blockDim.x;
                    if (v < VT) {
                        if (PACKED) {
                            prow[v] = (int32_t)(((uint32_t)p[k] & 0xFFFFu) |
                                                ((uint32_t)pt[k] << 16));
                        } else {
                            prow[v] = p[k];
                            trow[v] = pt[k];
                        }
                        if (HOPS) put_hop(out_hops, hb + v, hp[k], flags);
                    }
                }
            }
        } else
        for (int v0 = threadIdx.x; v0 < V; v0 += UF * blockDim.x) {
            int p[UF], sl[UF], pt[UF];
#pragma unroll
            for (int k = 0; k < UF; ++k) {
                const int v = v0 + k * (int)blockDim.x;
                p[k] = -1;
                sl[k] = -1;
                if (v < V && ((vis[v >> 5] >> (v & 31)) & 1u)) {
                    if (C16) {
                        p[k] = (int)ps16[swz(v)];
                        if (v != s) sl[k] = (int)sl8[swz(v)];
                    } else {
                        const uint32_t xx = ps[swz(v)];
                        p[k] = (int)(xx & 0xFFFFu);
                        if (v != s) sl[k] = (int)(xx >> 16);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < UF; ++k) {
                pt[k] = -1;
                if (sl[k] >= 0)
                    pt[k] = W > 0 ? ell_port[(size_t)p[k] * W + sl[k]] : port[row_ptr[p[k]] + sl[k]];
            }
#pragma unroll
            for (int k = 0; k < UF; ++k) {
                const int v = v0 + k * (int)blockDim.x;
                if (v < V) {
                    if (PACKED) {                // parent | port << 16, -1 -> 0xFFFF
                        prow[v] = (int32_t)(((uint32_t)p[k] & 0xFFFFu) |
                                            ((uint32_t)pt[k] << 16));
                    } else {
                        prow[v] = p[k];
                        trow[v] = pt[k];
                    }
                    if (HOPS) put_hop(out_hops, hb + v, p[k] < 0 ? -1 : (v == s ? 0 : (int)dep[v]),
                                      flags);
                }
            }
        }
        // the next source's init reuses the LDS state; a workgroup on its
        // last source (the headline: one source per workgroup) skips the
        // barrier, whose release fence waited for every table store of the
        // wave to be acknowledged (the flush measured 57.5 k of a 291 k-cycle
        // source life at 1,152 sources, 4.2 k at one: stamps)
        if (si + (int)gridDim.x < nsrc) __syncthreads();
#ifdef SDNR_STAMPS
        SDNR_STAMP(ph3);
        if (threadIdx.x == 0) {
            atomicAdd(&g_stamp[8], ph1 - ph0);       // init
            atomicAdd(&g_stamp[9], ph2 - ph1);       // search + worker tail
            atomicAdd(&g_stamp[10], ph3 - ph2);      // flush
        }
#endif
    }
#ifdef SDNR_STAMPS
    if (threadIdx.x == 0) {                      // span of the launch: last end, first start
        unsigned long long t;
        SDNR_STAMP(t);
        atomicMax(&g_stamp[11], t);
        atomicMax(&g_stamp[12], ~kstart);
    }
#endif
}

// slot trees from int32 ones: slot = position of v in parent's ascending CSR
// row (binary search); the root (parent == v) gets slot 63
__global__ __launch_bounds__(256) void dfs_slot_pack_kernel(size_t n, int V,
                                                            const int32_t *__restrict__ parent,
                                                            const int32_t *__restrict__ row_ptr,
                                                            const int32_t *__restrict__ col,
                                                            uint32_t *__restrict__ tree)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const int v = (int)(i % (size_t)V), p = parent[i];
        uint32_t t = 0xFFFFFFFFu;
        if (p == v) {
            t = (uint32_t)p | (63u << 26);
        } else if (p >= 0) {
            int lo = row_ptr[p], hi = row_ptr[p + 1];
            const int base = lo;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (col[mid] < v) lo = mid + 1; else hi = mid;
            }
            t = (uint32_t)p | ((uint32_t)(lo - base) << 26);
        }
        tree[i] = t;
    }
}

// packed tables from int32 ones (strategies without a packed epilogue)
__global__ __launch_bounds__(256) void dfs_pack_kernel(size_t n, const int32_t *__restrict__ parent,
                                                       const int32_t *__restrict__ port,
                                                       uint32_t *__restrict__ tree)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x)
        tree[i] = ((uint32_t)parent[i] & 0xFFFFu) | ((uint32_t)port[i] << 16);
}

template <typename Kern>
void allow_full_lds(Kern kernel)
{
    sdnr_allow_lds(reinterpret_cast<const void *>(kernel), SDNR_MAX_LDS_PER_BLOCK);
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

// LDS bytes per source of the two strategies
static size_t dfs_lds_bytes_small(int V)
{
    const size_t VWp = (size_t)((((V + 31) >> 5) + 3) & ~3);
    return align16(4 * VWp + 8 * (size_t)V + 2 * (size_t)V);
}

static size_t dfs_lds_bytes_global(int V, int ring = kRing)
{
    const size_t VWp = (size_t)((((V + 31) >> 5) + 3) & ~3);
    return align16(4 * VWp + 8 * (size_t)ring);
}

// stack-ring entries of the lane-packed kernel: small rings leave room for
// more resident sources on large graphs (the torus search is a chain of
// ~14k non-leaf pops per source: throughput comes from sources in flight);
// SDNROUTE_DFS_RING=128|1024 overrides
static int packed_ring(int V, int W)
{
    if (const char *f = getenv("SDNROUTE_DFS_RING")) {
        const int r = atoi(f);
        if (r == 128 || r == 1024) return r;
    }
    return V > 16384 && W <= 8 ? 128 : 1024;
}

// stack entries checked per batch by the lane-packed kernel with 8 lanes per
// row: J = 1 (8 entries) or 2 (16).  On the torus 13.6k of 32.8k pops push
// children, so a batch rarely retires more than two entries: the narrower
// batch halves the row traffic per step (torus 32^3: 108 -> 99 ms).
// SDNROUTE_DFS_PACKED_J overrides
static int packed_j8(int V)
{
    if (const char *f = sdnr_tune_env("SDNROUTE_DFS_PACKED_J")) {
        const int j = atoi(f);
        if (j == 1 || j == 2) return j;
    }
    return V > 16384 ? 1 : 2;
}

namespace {

struct DfsArgs {
    int V, W;
    const int32_t *row_ptr, *col, *port, *src;
    int nsrc;
    int32_t *parent, *port_out, *hops;
    uint2 *spill;
    const int32_t *port_csr;
};

template <bool ELL, bool HOPS, int K>
void launch_batch(bool small, int grid, size_t lds, hipStream_t st, const DfsArgs &a)
{
    if (small) {
        auto k = dfs_lds_batch_kernel<ELL, HOPS, K>;
        allow_full_lds(k);
        hipLaunchKernelGGL(k, dim3(grid), dim3(64), lds, st, a.V, a.W, a.row_ptr, a.col, a.port,
                           a.src, a.nsrc, a.parent, a.port_out, a.hops);
    } else {
        auto k = dfs_global_batch_kernel<ELL, HOPS, K>;
        allow_full_lds(k);
        hipLaunchKernelGGL(k, dim3(grid), dim3(64), lds, st, a.V, a.W, a.row_ptr, a.col, a.port,
                           a.src, a.nsrc, a.parent, a.port_out, a.hops, a.spill);
    }
}

template <bool ELL, bool HOPS>
void launch_batch_k(int K, bool small, int grid, size_t lds, hipStream_t st, const DfsArgs &a)
{
    if (K >= 16) launch_batch<ELL, HOPS, 16>(small, grid, lds, st, a);
    else if (K >= 8) launch_batch<ELL, HOPS, 8>(small, grid, lds, st, a);
    else if (K >= 4) launch_batch<ELL, HOPS, 4>(small, grid, lds, st, a);
    else launch_batch<ELL, HOPS, 1>(small, grid, lds, st, a);
}

template <bool HOPS>
void launch_wide(bool small, int grid, size_t lds, hipStream_t st, const DfsArgs &a)
{
    if (small) {
        auto k = dfs_lds_wide_kernel<false, HOPS>;
        allow_full_lds(k);
        hipLaunchKernelGGL(k, dim3(grid), dim3(64), lds, st, a.V, a.W, a.row_ptr, a.col, a.port,
                           a.src, a.nsrc, a.parent, a.port_out, a.hops);
    } else {
        auto k = dfs_global_wide_kernel<false, HOPS>;
        allow_full_lds(k);
        hipLaunchKernelGGL(k, dim3(grid), dim3(64), lds, st, a.V, a.W, a.row_ptr, a.col, a.port,
                           a.src, a.nsrc, a.parent, a.port_out, a.hops, a.spill);
    }
}

}  // namespace

static size_t dfs_lds_bytes_count(int V, bool hops)
{
    const size_t VWp = (size_t)((((V + 1 + 31) >> 5) + 3) & ~3);
    const size_t CWp = (size_t)((V + 1 + 3) & ~3);
    const size_t SWp = (size_t)((((V + 1) >> 1) + 3) & ~3);
    return align16(4 * (VWp + CWp + SWp) + 4 * (size_t)V + (hops ? 2 * (size_t)V : 0));
}

// quot: V is a twin-class quotient's, and dfs_async_kernel keeps the words of
// its flush behind the control words: an offset per class and the source's
// port row (SDNR_QUOT_FLUSH)
static size_t dfs_lds_bytes_async(int V, bool hops, bool c16 = false, bool quot = false)
{
    const size_t VWp = (size_t)((((V + 1 + 31) >> 5) + 3) & ~3);
    const size_t CWp = (size_t)(((((c16 ? (V + 2) >> 1 : V + 1) + 31) & ~31) + 64 + 255) & ~255);
    const size_t SWp = (size_t)((((V + 1) >> 1) + 3) & ~3);
    const size_t PW = (size_t)((V + 255) & ~255);
    const size_t PWp = c16 ? PW / 2 + PW / 4 : PW;
    return align16(4 * (VWp + CWp + SWp) + 4 * PWp +
                   (hops ? 4 * (size_t)((V + 1) >> 1) : 0) + 2 * 512 + 4 * 16 +
                   (quot && (SDNR_QUOT_FLUSH & 3) ? 4 * (size_t)((V + 3) & ~3) + 4 * SDNR_WAVE : 0));
}

// what a launch of dfs_async_kernel reserves: the graph's layout, also where
// the kernel lays out the quotient's (a fat tree's is well under half of it,
// so the flush's words cost the headline nothing); more only where a quotient
// of nearly the graph's size does not fit that with its flush's words.  The
// limit check and the workgroups per CU are computed from this
static size_t dfs_async_reserve(const sdnr_ctx *ctx, bool hops, bool c16, bool quot)
{
    const size_t g = dfs_lds_bytes_async(ctx->V, hops, c16);
    const size_t q = quot ? dfs_lds_bytes_async(ctx->q_V, hops, c16, true) : 0;
    return q > g ? q : g;
}

static size_t dfs_lds_bytes_coop(int V)
{
    const size_t VWp = (size_t)((((V + 1 + 31) >> 5) + 3) & ~3);
    return align16(4 * VWp + 8 * (size_t)V + 4 * (size_t)((V + 1) >> 1) + 4 * 32);
}

namespace {

template <bool HOPS, int KW>
void launch_coop_kw(int grid, size_t lds, hipStream_t st, int V, const uint16_t *adj,
                    const DfsArgs &a)
{
    auto k = dfs_coop_kernel<4, KW, HOPS>;
    allow_full_lds(k);
    hipLaunchKernelGGL(k, dim3(grid), dim3(4 * 64), lds, st, V, adj, a.row_ptr,
                       a.port_csr, a.src, a.nsrc, a.parent, a.port_out,
                       a.hops);
}

template <bool HOPS>
void launch_coop(int kw, int grid, size_t lds, hipStream_t st, int V, const uint16_t *adj,
                 const DfsArgs &a)
{
    if (kw >= 8) launch_coop_kw<HOPS, 8>(grid, lds, st, V, adj, a);
    else if (kw >= 4) launch_coop_kw<HOPS, 4>(grid, lds, st, V, adj, a);
    else launch_coop_kw<HOPS, 2>(grid, lds, st, V, adj, a);
}

}  // namespace

// slots per wave of the cooperative kernel (4 waves): SDNROUTE_DFS_COOP_KW
static int dfs_coop_kw()
{
    if (const char *f = sdnr_tune_env("SDNROUTE_DFS_COOP_KW")) {
        const int k = atoi(f);
        if (k == 2 || k == 4 || k == 8) return k;
    }
    return 4;
}

#ifdef SDNR_STAMPS
extern "C" int sdnr_debug_stamps(unsigned long long *out16)
{
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamp), 16 * sizeof(unsigned long long)) !=
        hipSuccess)
        return -5;
    unsigned long long z[16] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamp), z, sizeof z) == hipSuccess ? 0 : -5;
}
#endif

// waves per source of the asynchronous kernel: SDNROUTE_DFS_ASYNC_WAVES=2|3|4
// waves per source of the async kernel: 1 search + decrement workers, whose
// work per child is its in-degree -- 3 workers for rows of 33-64 neighbours
// (k=48: 0.116 ms vs 0.138 with 2), 2 for rows of <= 32 (dragonfly, 23
// neighbours: 0.289 vs 0.300 ms with 3); SDNROUTE_DFS_ASYNC_WAVES=2..6
static int dfs_async_waves(const sdnr_ctx *ctx, int nsrc)
{
    if (const char *f = getenv("SDNROUTE_DFS_ASYNC_WAVES")) {
        const int k = atoi(f);
        if ((k >= 2 && k <= 6) || k == 8) return k;
    }
    // at most ~2 sources per CU (one GPU's share of a multi-GPU step, single
    // sources): 5 decrement workers keep the counts fresher and the search
    // wave still has its SIMD mostly to itself -- k=48 1 / 144 / 256 / 288
    // sources 63.4 / 64.3 / 65.1 / 69.1 -> 56.8 / 58.4 / 59.4 / 64.2 us,
    // dragonfly 258 sources 127.7 -> 120.8 us; equal at 576 sources, and
    // slower once every CU holds several sources (k=48 1,152: 91.6 -> 137 us
    // with 4 workers), where the workers compete with the search waves.
    // Round 4: with the dword-paired rows (in-degree > 32) 7 workers -- k=48
    // 144 / 1 sources 48.8 / 47.1 -> 46.9 / 45.1 us.  nsrc: the searches
    // that run -- a folded search's published live count where dfs_dispatch
    // has one (k=48 1,152 sources, 48 live: 63.4 -> 56.4 us at 8, 58.1 at 6)
    if (nsrc <= 2 * ctx->num_cus) return ctx->radj_pair ? 6 : 8;
    return ctx->max_deg <= 32 ? 3 : 4;
}

// waves per source of the counted-pop kernel: SDNROUTE_DFS_COUNT_WAVES=2|4|6
static int dfs_count_waves()
{
    if (const char *f = sdnr_tune_env("SDNROUTE_DFS_COUNT_WAVES")) {
        const int k = atoi(f);
        if (k == 2 || k == 4 || k == 6) return k;
    }
    return 4;
}

// SDNROUTE_DFS_PACKED=0 disables the lane-packed large-graph kernel
static bool packed_ok()
{
    const char *f = getenv("SDNROUTE_DFS_PACKED");
    return !(f && !strcmp(f, "0"));
}

// pops checked per batch: wide rows make each leaf pop expensive, so batch
// deeper; SDNROUTE_DFS_BATCH=1|4|8|16 overrides (tuning / tests)
static int dfs_batch_depth(const sdnr_ctx *ctx)
{
    if (const char *f = sdnr_tune_env("SDNROUTE_DFS_BATCH")) {
        const int k = atoi(f);
        if (k == 1 || k == 4 || k == 8 || k == 16) return k;
    }
    return ctx->max_deg >= 12 ? 16 : 8;
}

static int dfs_flags(int dflt = 0)
{
    const char *f = sdnr_tune_env("SDNROUTE_DFS_FLAGS");
    const int v = f ? atoi(f) : dflt;
#ifdef SDNR_DIAG_VARIANTS
    return v;
#else
    // the timing diagnostics that leave the tables wrong (no stores, no port
    // lookups) exist only in the diagnostic build
    return v & ~(kFlagNoStore | kFlagNoPort);
#endif
}

// SDNROUTE_DFS_SPLIT=0 keeps the single-wave lane-packed kernel (A/B, tests)
static bool split_ok()
{
    const char *f = getenv("SDNROUTE_DFS_SPLIT");
    return !(f && !strcmp(f, "0"));
}

// search / writer split kernel (large graphs, rows of <= 32 slots); records
// the end event itself
template <int NS>
static int launch_split_ns(sdnr_ctx *ctx, const int32_t *d_src, int32_t nsrc, int32_t *d_parent,
                           int32_t *d_port, int32_t *d_hops, uint32_t *d_tree, int tree,
                           int hflags);

// search waves per workgroup: 7 on sparse tori (4 workgroups of 8 waves fill
// a CU's 32 wave slots with 28 sources), else 3 (LDS-bound: Jellyfish fits 3
// workgroups of 3 sources); SDNROUTE_DFS_SPLIT_NS=3|7 overrides
static int launch_split(sdnr_ctx *ctx, const int32_t *d_src, int32_t nsrc, int32_t *d_parent,
                        int32_t *d_port, int32_t *d_hops, uint32_t *d_tree, int tree, int hflags)
{
    int ns = ctx->W <= 8 && packed_j8(ctx->V) == 1 ? 7 : 3;
    if (ctx->W > 8 && ctx->W <= 16) {
        // rows of 9-16 slots (Jellyfish): 3 or 5 sources per workgroup,
        // whichever keeps more sources resident per CU (100k Jellyfish
        // without hop counts: 2 x 5 = 10 vs 3 x 3 = 9, measured 5 % faster)
        const bool hops = d_hops != nullptr;
        auto per_cu = [&](int k) {
            const size_t l = split_lds_words(ctx->V, 512, k, hops, 16) * 4;
            size_t b = SDNR_LDS_PER_CU / l;
            if (b > (size_t)(32 / (k + 1))) b = 32 / (k + 1);
            return (size_t)k * b;
        };
        if (per_cu(5) > per_cu(3)) ns = 5;
    }
    if (const char *f = getenv("SDNROUTE_DFS_SPLIT_NS")) {
        const int k = atoi(f);
        if (k == 3 || k == 7) ns = k;
        if ((k == 5 || k == 11) && ctx->W > 8 && ctx->W <= 16) ns = k;   // rows of 9-16 slots
    }
    switch (ns) {
    case 7: return launch_split_ns<7>(ctx, d_src, nsrc, d_parent, d_port, d_hops, d_tree, tree,
                                     hflags);
    case 5: return launch_split_ns<5>(ctx, d_src, nsrc, d_parent, d_port, d_hops, d_tree, tree,
                                     hflags);
    case 11: return launch_split_ns<11>(ctx, d_src, nsrc, d_parent, d_port, d_hops, d_tree, tree,
                                      hflags);
    default: return launch_split_ns<3>(ctx, d_src, nsrc, d_parent, d_port, d_hops, d_tree, tree,
                                     hflags);
    }
}

template <int NS>
static int launch_split_ns(sdnr_ctx *ctx, const int32_t *d_src, int32_t nsrc, int32_t *d_parent,
                           int32_t *d_port, int32_t *d_hops, uint32_t *d_tree, int tree,
                           int hflags)
{
    const int V = ctx->V, W = ctx->W;
    const bool packed = d_tree != nullptr, hops = d_hops != nullptr;
    const int lpr = W <= 8 ? 8 : (W <= 16 ? 16 : 32);
    const int j8 = packed_j8(V);
    // stack ring: 128 entries on sparse tori (more sources per CU), 512 for
    // rows of 9-32 slots (Jellyfish: 3 workgroups of 3 sources per CU)
    int ring = lpr == 8 ? (j8 == 1 ? 128 : 1024) : 512;
    if (const char *f = getenv("SDNROUTE_DFS_SPLIT_RING"))   // rows of 9-16 slots
        if (lpr == 16 && !strcmp(f, "256")) ring = 256;
    constexpr bool kWide = NS == 5 || NS == 11;   // only for rows of 9-16 slots
    if (kWide && lpr != 16) return sdnr_fail(SDNR_ERR_INVAL, "dfs split: NS=%d needs rows of 9-16 slots", NS);
    const int fmt = ctx->ell16 && V <= 65535 ? kRow16 : (ctx->ell16 && ctx->ell_hi ? kRow17 : kRow32);
    if (tree == kTreePort16 && fmt != kRow16)
        return sdnr_fail(SDNR_ERR_INVAL, "dfs split: packed tables need V <= 65535");
    if (tree == kTreeSlot && hops && fmt == kRow32)
        return sdnr_fail(SDNR_ERR_INVAL, "dfs split: slot trees with hop counts need V <= 131071");
    // dictionary rows where the upload built them (rows of <= 8 slots)
    const bool dict = ctx->dict_bp && lpr == 8 && !kWide;
    const size_t dict_words =
        dict ? (size_t)ctx->dict_bpw + 8 * (size_t)ctx->dict_NB + 8 * (size_t)ctx->dict_P : 0;
    const size_t lds = (split_lds_words(V, ring, NS, hops, lpr, dict) + dict_words) * 4;
    if (lds > SDNR_MAX_LDS_PER_BLOCK)
        return sdnr_fail(SDNR_ERR_INVAL, "graph too large for the LDS visited sets (V=%d)", V);
    size_t bpc = SDNR_LDS_PER_CU / lds;
    if (bpc > (size_t)(32 / (NS + 1))) bpc = 32 / (NS + 1);    // 32 wave slots per CU
    if (bpc < 1) bpc = 1;
    int grid = (int)((size_t)ctx->num_cus * bpc);
    const int need = (nsrc + NS - 1) / NS;
    if (grid > need) grid = need;
    int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes,
                          (size_t)grid * NS * (size_t)V * sizeof(uint2));
    if (rc) return rc;
    uint2 *spill = static_cast<uint2 *>(ctx->scratch);
    const void *rows = fmt == kRow32 ? static_cast<const void *>(ctx->ell_col)
                                     : static_cast<const void *>(ctx->ell16);
    int32_t *par = packed ? reinterpret_cast<int32_t *>(d_tree) : d_parent;
    static const char *names[4][3] = {
        {"dfs_split_kernel<row32>", "dfs_split_kernel<row32>", "dfs_split_kernel<row32,slots>"},
        {"dfs_split_kernel<row16>", "dfs_split_kernel<row16,packed>", "dfs_split_kernel<row16,slots>"},
        {"dfs_split_kernel<row17>", "dfs_split_kernel<row17>", "dfs_split_kernel<row17,slots>"},
        {"dfs_split_kernel<dict>", "dfs_split_kernel<dict,packed>", "dfs_split_kernel<dict,slots>"}};
    ctx->last_kernel = names[dict ? kRowDict : fmt][tree];
    // rows of 9-16 slots (Jellyfish): search waves issue at raised priority
    // over their writer (measured 1.027 -> 0.973 s on the 100k Jellyfish; the
    // torus rows of 6 slots measured 3 % slower with it, so not there)
    int flags = dfs_flags(lpr == 16 ? kFlagPrio : 0) | hflags;
    // sources by CU chunk (kFlagCuMap; SDNROUTE_DFS_CUMAP=0|1 overrides):
    // same box A/B, torus 32^3 99.6 -> 86.4 ms, Jellyfish 100k 976 -> 883 ms
    bool cumap = true;
    if (const char *f = getenv("SDNROUTE_DFS_CUMAP")) cumap = !strcmp(f, "1");
    const int nch = ctx->num_cus;
    int *wq = nullptr;
    if (cumap) {
        flags |= kFlagCuMap;
        rc = sdnr_reserve(&ctx->wq, &ctx->wq_bytes, (size_t)(nch + 1 + 1024) * sizeof(int));
        if (rc) return rc;
        wq = static_cast<int *>(ctx->wq);
        SDNR_HIP(hipMemsetAsync(wq, 0, (size_t)(nch + 1) * sizeof(int), ctx->stream));
        SDNR_HIP(hipMemsetAsync(wq + nch + 1, 0xFF, 1024 * sizeof(int), ctx->stream));
    }
#define SDNR_SPLIT(L_, J_, R_, H_, F_, P_)                                                    \
    do {                                                                                     \
        auto k = dfs_split_kernel<L_, J_, H_, R_, NS, F_, P_>;                               \
        sdnr_allow_lds(reinterpret_cast<const void *>(k), lds);                              \
        hipLaunchKernelGGL(k, dim3(grid), dim3((NS + 1) * 64), lds, ctx->stream, V, W, rows,     \
                           ctx->ell_hi, ctx->ell_port, d_src, nsrc, par, d_port, d_hops,     \
                           spill, ctx->d_err, flags, wq, nch, ctx->dict_bp, ctx->dict_bt,    \
                           ctx->dict_off, ctx->dict_bpw, ctx->dict_NB, ctx->dict_P);         \
    } while (0)
#define SDNR_SPLIT_F(L_, J_, R_, H_)                                                          \
    do {                                                                                     \
        if constexpr (L_ == 8 && !kWide) {                                                   \
            if (dict) {                                                                      \
                if (tree == kTreeSlot) SDNR_SPLIT(L_, J_, R_, H_, kRowDict, kTreeSlot);      \
                else if (packed) SDNR_SPLIT(L_, J_, R_, H_, kRowDict, kTreePort16);          \
                else SDNR_SPLIT(L_, J_, R_, H_, kRowDict, kTreeInt32);                       \
                break;                                                                       \
            }                                                                                \
        }                                                                                    \
        if (tree == kTreeSlot) {                                                             \
            if (fmt == kRow16) SDNR_SPLIT(L_, J_, R_, H_, kRow16, kTreeSlot);                \
            else if (fmt == kRow17) SDNR_SPLIT(L_, J_, R_, H_, kRow17, kTreeSlot);           \
            else if constexpr (!H_) SDNR_SPLIT(L_, J_, R_, H_, kRow32, kTreeSlot);           \
            break;                                                                           \
        }                                                                                    \
        if (fmt == kRow16 && packed) SDNR_SPLIT(L_, J_, R_, H_, kRow16, kTreePort16);        \
        else if (fmt == kRow16) SDNR_SPLIT(L_, J_, R_, H_, kRow16, kTreeInt32);              \
        else if (fmt == kRow17) SDNR_SPLIT(L_, J_, R_, H_, kRow17, kTreeInt32);              \
        else SDNR_SPLIT(L_, J_, R_, H_, kRow32, kTreeInt32);                                 \
    } while (0)
#define SDNR_SPLIT_H(L_, J_, R_)                                                              \
    do {                                                                                     \
        if (hops) SDNR_SPLIT_F(L_, J_, R_, true); else SDNR_SPLIT_F(L_, J_, R_, false);      \
    } while (0)
    if constexpr (kWide) {
        // stack entries per window: 8 (J = 2; SDNROUTE_DFS_SPLIT_J=4|1 for 16 |
        // 4).  Same box, 100k Jellyfish, all sources (gpurun_out/r5_jfj2): 16
        // entries 880 ms, 8 entries 833 ms, 4 entries 875 ms -- the window's
        // row loads (the CU's data return is ~90 % busy) against the leaf
        // skips a narrower window takes more iterations for
        const char *jf = getenv("SDNROUTE_DFS_SPLIT_J");
        const int jw = jf && (atoi(jf) == 4 || atoi(jf) == 1) ? atoi(jf) : 2;
        if (ring == 256) SDNR_SPLIT_H(16, 4, 256);
        else if (jw == 2) SDNR_SPLIT_H(16, 2, 512);
        else if (jw == 1) SDNR_SPLIT_H(16, 1, 512);
        else SDNR_SPLIT_H(16, 4, 512);
    } else {
        if (lpr == 8 && ring == 128) SDNR_SPLIT_H(8, 1, 128);
        else if (lpr == 8) SDNR_SPLIT_H(8, 2, 1024);
        else if (lpr == 16 && ring == 256) SDNR_SPLIT_H(16, 4, 256);
        else if (lpr == 16) SDNR_SPLIT_H(16, 4, 512);
        else SDNR_SPLIT_H(32, 8, 512);
    }
#undef SDNR_SPLIT_H
#undef SDNR_SPLIT_F
#undef SDNR_SPLIT
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}

int sdnr_launch_tree_pack(sdnr_ctx *ctx, const int32_t *parent, const int32_t *port, size_t n,
                          uint32_t *tree, bool slots)
{
    const int V = ctx->V;
    if (slots)
        hipLaunchKernelGGL(dfs_slot_pack_kernel, dim3(ctx->num_cus * 8), dim3(256), 0,
                           ctx->stream, n, V, parent, ctx->row_ptr, ctx->col, tree);
    else
        hipLaunchKernelGGL(dfs_pack_kernel, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream,
                           n, parent, port, tree);
    SDNR_HIP(hipGetLastError());
    return SDNR_OK;
}

#ifdef SDNR_DIAG_VARIANTS
// the register-visited kernel (dfs_bits.hip) where it applies: forced with
// SDNROUTE_DFS_STRATEGY=bits (A/B; not yet the default)
static bool dfs_bits_default(const char *force)
{
    return force && !strcmp(force, "bits");
}

#endif

// the async kernel for a row form: compact LDS (C16), paired in-rows,
// dword-paired in-rows, or plain u16 in-rows
template <int N_, bool H_, bool P_, bool SPEC, bool Q_ = false>
static auto async_pick(bool c16, bool pair, bool dw)
{
    // (SPEC: the plain-row kernel only -- the compact / paired forms, the
    // dragonfly's, measured slower with the speculative pop compiled in:
    // 2,064 sources 177.3 -> 180.4 us, gpurun_out/r5_abspec)
    return c16 ? (pair ? dfs_async_kernel<N_, H_, P_, true, 1, false, Q_>
                       : dfs_async_kernel<N_, H_, P_, true, 0, false, Q_>)
               : (pair ? dfs_async_kernel<N_, H_, P_, false, 1, false, Q_>
                       : (dw ? dfs_async_kernel<N_, H_, P_, false, 2, false, Q_>
                             : dfs_async_kernel<N_, H_, P_, false, 0, SPEC, Q_>));
}

// hop counts as u16 (0xFFFF unreached) into d_hops
__global__ __launch_bounds__(256) void dfs_hops16_kernel(size_t n, const int32_t *__restrict__ h,
                                                         uint16_t *__restrict__ out)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x)
        out[i] = (uint16_t)h[i];
}

// the visited set and the stack of one search fit the LDS strategies
static bool dfs_small(const sdnr_ctx *ctx, int nsrc)
{
    const int V = ctx->V;
    const size_t small_b = dfs_lds_bytes_small(V);
    const size_t cu_blocks_small = SDNR_LDS_PER_CU / small_b;
    bool small = V < 65536 && small_b <= 64 * 1024 &&
                 (small_b <= 40 * 1024 ||
                  (size_t)nsrc <= (size_t)ctx->num_cus * cu_blocks_small);
    // debug/test knob: SDNROUTE_DFS_STRATEGY=lds|global forces a strategy
    if (const char *f = getenv("SDNROUTE_DFS_STRATEGY")) {
        if (!strcmp(f, "global")) small = false;
        else if ((!strcmp(f, "lds") || !strcmp(f, "coop") || !strcmp(f, "count") ||
                  !strcmp(f, "async")) && V < 65536 &&
                 small_b <= SDNR_MAX_LDS_PER_BLOCK)
            small = true;
    }
    return small;
}

// the counted-pop kernels apply; async: dfs_async_kernel is the strategy
static bool dfs_count_ok(const sdnr_ctx *ctx, bool hops)
{
    return ctx->adj16 != nullptr && ctx->radj16 != nullptr && ctx->V < 65535 &&
           dfs_lds_bytes_count(ctx->V, hops) <= SDNR_MAX_LDS_PER_BLOCK;
}

static bool dfs_async(const sdnr_ctx *ctx, int nsrc, bool hops)
{
    const char *force = getenv("SDNROUTE_DFS_STRATEGY");
    return dfs_count_ok(ctx, hops) &&
           dfs_lds_bytes_async(ctx->V, hops) <= SDNR_MAX_LDS_PER_BLOCK &&
           (force ? !strcmp(force, "async") : dfs_small(ctx, nsrc));
}

// search the twin-class quotient (ctx->q_*, capi.hip) in
// place of the graph?  Only a graph with twins has one, and by default it is
// taken when it has at most half the graph's links: below that the search
// saves little and the flush's two extra gathers per vertex are not paid for
// (a fat tree's quotient has 1 / k of the links; a graph with one pair of
// twins stays on its own rows).  SDNROUTE_DFS_QUOTIENT=0|1 forces it off / on
// (A/B, tests on graphs under the rule)
static bool dfs_quotient(const sdnr_ctx *ctx, bool hops)
{
    if (!ctx->q_tab || ctx->q_V <= 0) return false;
    // (a quotient whose layout, with its flush's words, is beyond a
    // workgroup's LDS is none: the graph is searched on its own rows)
    if (dfs_async_reserve(ctx, hops, false, true) > SDNR_MAX_LDS_PER_BLOCK) return false;
    if (const char *f = getenv("SDNROUTE_DFS_QUOTIENT")) {
        if (!strcmp(f, "0")) return false;
        if (!strcmp(f, "1")) return true;
    }
    return 2 * (int64_t)ctx->q_E <= (int64_t)ctx->E;
}

// what the low-load form of the folded 4-wave search changes (A/B builds:
// -DSDNR_FOLD_LOW_FORM=n): 1 the speculative pop compiled out, 2 the
// dword-paired worker rows (their step width: SDNR_ASYNC_G_DW4)
#ifndef SDNR_FOLD_LOW_FORM
#define SDNR_FOLD_LOW_FORM 2
#endif

// the strategy dispatch: one search per entry of d_src.  d_live (device, may
// be null): only the first min(nsrc, *d_live) entries are searched and only
// their rows written -- honoured where dfs_takes_live() says so, else every
// entry is searched, so the caller pads the list with -1 (empty rows).
// live_n (with low; 0: none): the published live count the caller took the
// low-load form from -- dfs_async_kernel is then dispatched as live_n
// searches select it, not as nsrc does
static int dfs_dispatch(sdnr_ctx *ctx, const int32_t *d_src, int32_t nsrc,
                        int32_t *d_parent, int32_t *d_port, int32_t *d_hops, uint32_t *d_tree,
                        bool slots = false, bool hops16 = false,
                        const int32_t *d_live = nullptr, bool low = false, int32_t live_n = 0)
{
    const int V = ctx->V;
    if (nsrc == 0 || V == 0) return SDNR_OK;
    const bool packed = d_tree != nullptr;
    const bool ell = ctx->W > 0;
    const bool hops = d_hops != nullptr;
    const bool narrow = ctx->max_deg <= SDNR_WAVE;     // one row = one wavefront
    const size_t small_b = dfs_lds_bytes_small(V);
    const bool small = dfs_small(ctx, nsrc);
    size_t lds = small ? small_b : dfs_lds_bytes_global(V);
    if (lds > SDNR_MAX_LDS_PER_BLOCK)
        return sdnr_fail(SDNR_ERR_INVAL, "graph too large for the LDS visited set (V=%d)", V);
    size_t bpc = SDNR_LDS_PER_CU / lds;
    if (bpc > 16) bpc = 16;
    if (bpc < 1) bpc = 1;
    int grid = (int)((size_t)ctx->num_cus * bpc);
    if (grid > nsrc) grid = nsrc;
    uint2 *spill = nullptr;
    if (!small) {
        const size_t need = (size_t)grid * (size_t)V * sizeof(uint2);
        int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, need);
        if (rc) return rc;
        spill = static_cast<uint2 *>(ctx->scratch);
    }
    DfsArgs a{V, ctx->W, ctx->row_ptr, ell ? ctx->ell_col : ctx->col,
              ell ? ctx->ell_port : ctx->port, d_src, nsrc, d_parent, d_port, d_hops, spill,
              ctx->port};
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    const char *force = getenv("SDNROUTE_DFS_STRATEGY");
#ifdef SDNR_DIAG_VARIANTS
    // diagnostic build only (tools/diag/build_diag.sh): the two losing
    // variants of DESIGN.md 4.1a / 4.1b, forced by SDNROUTE_DFS_STRATEGY
    // rows in LDS as arithmetic runs (dfs_runs.hip), SDNROUTE_DFS_STRATEGY=
    // runs: measured no faster than dfs_async_kernel, so
    // opt-in
    if (!(slots && packed) && sdnr_dfs_runs_ok(ctx, hops) && force && !strcmp(force, "runs")) {
        int rc = sdnr_launch_dfs_runs(ctx, d_src, nsrc, d_parent, d_port, d_hops, d_tree);
        if (rc) return rc;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
        return SDNR_OK;
    }
    // bitmap rows, visited set in registers (dfs_bits.hip): V <= 4096;
    // SDNROUTE_DFS_STRATEGY=bits forces it (A/B), =async the round-3 kernel
    if (!slots && sdnr_dfs_bits_ok(ctx) && dfs_bits_default(force)) {
        int rc = sdnr_launch_dfs_bits(ctx, d_src, nsrc, d_parent, d_port, d_hops, d_tree, hops16);
        if (rc) return rc;
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
        return SDNR_OK;
    }
#endif
    const bool count_ok = dfs_count_ok(ctx, hops);
    const bool async = dfs_async(ctx, nsrc, hops);
    slots = slots && packed;
    const int hflags = hops && hops16 ? kFlagHops16 : 0;
    if (!async && !small && ell && ctx->W <= 32 && packed_ok() && split_ok() &&
        (!packed || slots || (ctx->ell16 && V <= 65535)) &&
        !(slots && hops && !(ctx->ell16 && (V <= 65535 || ctx->ell_hi))))
        return launch_split(ctx, d_src, nsrc, d_parent, d_port, d_hops, d_tree,
                            slots ? kTreeSlot : (packed ? kTreePort16 : kTreeInt32), hflags);
    if ((packed && (!async || slots)) || (hops && hops16 && !async)) {
        // no such epilogue in this strategy: int32 tables into scratch, then
        // pack (and narrow the hop counts)
        const size_t n = (size_t)nsrc * (size_t)V;
        const bool h16 = hops && hops16;
        int rc = sdnr_reserve(&ctx->scratch2, &ctx->scratch2_bytes,
                              (h16 ? 3 : 2) * n * sizeof(int32_t));
        if (rc) return rc;
        int32_t *tp = static_cast<int32_t *>(ctx->scratch2);
        int32_t *th = h16 ? tp + 2 * n : d_hops;
        if (!packed) {                           // int32 tables, u16 hop counts
            if ((rc = dfs_dispatch(ctx, d_src, nsrc, d_parent, d_port, tp, nullptr))) return rc;
            hipLaunchKernelGGL(dfs_hops16_kernel, dim3(ctx->num_cus * 8), dim3(256), 0,
                               ctx->stream, n, tp, reinterpret_cast<uint16_t *>(d_hops));
            SDNR_HIP(hipGetLastError());
            if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
            return SDNR_OK;
        }
        if ((rc = dfs_dispatch(ctx, d_src, nsrc, tp, tp + n, th, nullptr))) return rc;
        if (h16)
            hipLaunchKernelGGL(dfs_hops16_kernel, dim3(ctx->num_cus * 8), dim3(256), 0,
                               ctx->stream, n, th, reinterpret_cast<uint16_t *>(d_hops));
        if (slots)
            hipLaunchKernelGGL(dfs_slot_pack_kernel, dim3(ctx->num_cus * 8), dim3(256), 0,
                               ctx->stream, n, V, tp, ctx->row_ptr, ctx->col, d_tree);
        else
            hipLaunchKernelGGL(dfs_pack_kernel, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream,
                               n, tp, tp + n, d_tree);
        SDNR_HIP(hipGetLastError());
        if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
        return SDNR_OK;
    }
    const bool count = !async && count_ok && (force ? !strcmp(force, "count") : small);
    const bool coop_ok = ctx->adj16 != nullptr && V < 65535 &&
                         dfs_lds_bytes_coop(V) <= SDNR_MAX_LDS_PER_BLOCK;
    const bool coop = !count && coop_ok && (force ? !strcmp(force, "coop") : small);
    if (async) {
        int *err = ctx->d_err;
        // the search runs on the twin-class quotient where that is worth
        // taking (dfs_quotient): the quotient's rows in every form the
        // graph's come in, so all the rules below read as they do without it
        const bool quot = dfs_quotient(ctx, hops);
        ctx->dfs_quotient = quot;
        // workgroups per CU at w waves: LDS, and the 32 wave slots; the
        // compact layout (u16 counts, u16 parents + u8 slots) where it holds
        // more sources at once and the full layout cannot hold them all
        // (dragonfly 2,064 sources: 9 x 3 waves per CU vs 6);
        // SDNROUTE_DFS_C16=0|1 forces it
        auto per_cu = [&](int w, bool c) {
            size_t b = SDNR_LDS_PER_CU / dfs_async_reserve(ctx, hops, c, quot);
            if (b > (size_t)(32 / w)) b = 32 / w;
            return b < 1 ? (size_t)1 : b;
        };
        auto compact = [&](int w) {
            bool c = per_cu(w, true) > per_cu(w, false) &&
                     (size_t)ctx->num_cus * per_cu(w, false) < (size_t)nsrc;
            if (const char *f = getenv("SDNROUTE_DFS_C16")) c = !strcmp(f, "1");
            return c;
        };
        // pre-swizzled worker rows (SDNROUTE_DFS_PRESWZ=0 keeps the plain ones)
        const char *pz = getenv("SDNROUTE_DFS_PRESWZ");
        auto rows_of = [&](bool c) {
            return quot ? (c ? ctx->q_radjc : ctx->q_radjw) : (c ? ctx->radjc : ctx->radjw);
        };
        auto preswz_of = [&](bool c) { return rows_of(c) && !(pz && !strcmp(pz, "0")); };
        // the wave count: the caller's nsrc selects it, or -- the folded
        // search in its low-load form, taken from a published live count --
        // that count (48 live searches of 1,152 sources: 7 workers each, not
        // 3), where the rows are then neither compact nor paired; all that
        // follows from nw follows it
        int nw = dfs_async_waves(ctx, nsrc);
        if (low && d_live && live_n > 0) {
            const int cw = dfs_async_waves(ctx, live_n);
            const bool cc = compact(cw);
            if (!cc && !(preswz_of(cc) && ctx->radj_pair)) nw = cw;
        }
        const bool c16 = compact(nw);
        const size_t cl = dfs_async_reserve(ctx, hops, c16, quot);
        const size_t cpc = per_cu(nw, c16);
        const uint16_t *rw = rows_of(c16);
        const bool preswz = preswz_of(c16);
        // speculative stack pops (SDNROUTE_DFS_SPECPOP=0|1).
        // Compiled into the 4-wave plain-row kernel only (the k=48
        // headline's regime: 1,152 sources 83.0 -> 82.3 us, same ISA with
        // the pop off / on): its code cost the 8-wave low-load kernel ~8 us
        // even switched off, and the dragonfly's 3-wave compact kernel 1-2 %
        // (see dfs_async_kernel's SPEC; gpurun_out/r5_abr4, r5_abspec)
        bool specpop = true;
        if (const char *f = getenv("SDNROUTE_DFS_SPECPOP")) specpop = !strcmp(f, "1");
        bool spec = specpop;
        const int aflags = dfs_flags(kFlagPrio) | (preswz ? kFlagPreSwz : 0) | hflags |
                           (specpop ? kFlagSpecPop : 0);
        // paired worker rows (in-degree <= 32, pre-swizzled rows only);
        // else, at <= 2 sources per CU (the 5-worker regime), dword-paired
        // rows: k=48 1 / 144 sources 56.3 / 57.8 -> 54.7 / 56.4 us; at the
        // 1,152-source headline they measured 0.0895 -> 0.1010 ms, so the
        // u16 rows stay there (SDNROUTE_DFS_DW=0|1 forces either)
        const bool pair = preswz && ctx->radj_pair;
        const char *dq = sdnr_tune_env("SDNROUTE_DFS_DW");
        bool dw = preswz && !pair && !c16 && nw >= 6;
        if (dq) dw = preswz && !pair && !c16 && !strcmp(dq, "1");
        // the folded search's low-load form (sdnr_launch_dfs asks for it when
        // few searches are live): another instantiation, bit-exact with the
        // full-load one.  A forced form has no count: nw, the grid and the
        // name stay the caller's nsrc's
        if (low && d_live && !c16 && !pair) {
            if (SDNR_FOLD_LOW_FORM & 1) spec = false;
            if (SDNR_FOLD_LOW_FORM & 2) dw = preswz;
            ctx->dfs_form = kDfsFormLow;
        }
        int cgrid = (int)((size_t)ctx->num_cus * cpc);
        // (a count-selected grid capped at kFoldLowPerCu per CU, 512 for 1,024
        // workgroups of which 48 search: 57.7 against 57.5 us, not kept)
        if (cgrid > nsrc) cgrid = nsrc;
        // the search wave issues at raised priority over the decrement
        // workers (dragonfly 0.316 -> 0.300 ms, k=48 unchanged)
        static const char *names[] = {"", "", "dfs_async_kernel<2>", "dfs_async_kernel<3>",
                                      "dfs_async_kernel<4>", "dfs_async_kernel<5>",
                                      "dfs_async_kernel<6>", "", "dfs_async_kernel<8>"};
        ctx->last_kernel = names[nw];
#define SDNR_ASYNC_P(N_, H_, P_)                                                             \
    do {                                                                                     \
        constexpr bool kSpecOk = N_ == 4;              /* the k=48 headline's regime */      \
        auto k = quot ? (spec && kSpecOk ? async_pick<N_, H_, P_, kSpecOk, true>(c16, pair, dw) \
                                         : async_pick<N_, H_, P_, false, true>(c16, pair, dw)) \
                      : (spec && kSpecOk ? async_pick<N_, H_, P_, kSpecOk>(c16, pair, dw)    \
                                         : async_pick<N_, H_, P_, false>(c16, pair, dw));    \
        allow_full_lds(k);                                                                   \
        hipLaunchKernelGGL(k, dim3(cgrid), dim3(N_ * 64), cl, ctx->stream,                   \
                           quot ? ctx->q_V : V, quot ? ctx->q_adj16 : ctx->adj16,            \
                           preswz ? rw : (quot ? ctx->q_radj16 : ctx->radj16),               \
                           quot ? ctx->q_deg32 : ctx->deg32, ctx->row_ptr,                   \
                           ctx->port, ctx->W, ctx->ell_port, d_src, nsrc,                    \
                           P_ ? reinterpret_cast<int32_t *>(d_tree) : d_parent, d_port,      \
                           d_hops, err, aflags, d_live,                                      \
                           quot ? ctx->q_tab : static_cast<const sdnr_quot *>(nullptr));     \
    } while (0)
#define SDNR_ASYNC(N_, H_) SDNR_ASYNC_P(N_, H_, false)
        if (packed) {
            static const char *pnames[] = {"", "", "dfs_async_kernel<2,packed>",
                                           "dfs_async_kernel<3,packed>",
                                           "dfs_async_kernel<4,packed>",
                                           "dfs_async_kernel<5,packed>",
                                           "dfs_async_kernel<6,packed>", "",
                                           "dfs_async_kernel<8,packed>"};
            ctx->last_kernel = pnames[nw];
            if (hops) {                          // the drop-in's pool: tree words + depth
                static const char *hnames[] = {"", "", "", "dfs_async_kernel<3,packed,hops>",
                                               "dfs_async_kernel<4,packed,hops>", "",
                                               "dfs_async_kernel<6,packed,hops>"};
                const int hw = nw <= 3 ? 3 : (nw >= 6 ? 6 : 4);
                ctx->last_kernel = hnames[hw];
                if (hw == 3) SDNR_ASYNC_P(3, true, true);
                else if (hw == 6) SDNR_ASYNC_P(6, true, true);
                else SDNR_ASYNC_P(4, true, true);
            } else if (nw == 2) SDNR_ASYNC_P(2, false, true);
            else if (nw == 3) SDNR_ASYNC_P(3, false, true);
            else if (nw == 5) SDNR_ASYNC_P(5, false, true);
            else if (nw == 6) SDNR_ASYNC_P(6, false, true);
            else if (nw == 8) SDNR_ASYNC_P(8, false, true);
            else SDNR_ASYNC_P(4, false, true);
        } else if (nw == 2) {
            if (hops) SDNR_ASYNC(2, true); else SDNR_ASYNC(2, false);
        } else if (nw == 3) {
            if (hops) SDNR_ASYNC(3, true); else SDNR_ASYNC(3, false);
        } else if (nw == 5) {
            if (hops) SDNR_ASYNC(5, true); else SDNR_ASYNC(5, false);
        } else if (nw == 6) {
            if (hops) SDNR_ASYNC(6, true); else SDNR_ASYNC(6, false);
        } else if (nw == 8) {
            if (hops) SDNR_ASYNC(8, true); else SDNR_ASYNC(8, false);
        } else {
            if (hops) SDNR_ASYNC(4, true); else SDNR_ASYNC(4, false);
        }
#undef SDNR_ASYNC
#undef SDNR_ASYNC_P
    } else if (count) {
        const size_t cl = dfs_lds_bytes_count(V, hops);
        size_t cpc = SDNR_LDS_PER_CU / cl;
        if (cpc > 8) cpc = 8;
        if (cpc < 1) cpc = 1;
        int cgrid = (int)((size_t)ctx->num_cus * cpc);
        if (cgrid > nsrc) cgrid = nsrc;
        const int nw = dfs_count_waves();
        ctx->last_kernel = nw == 2 ? "dfs_count_kernel<2>" : nw == 6 ? "dfs_count_kernel<6>"
                                                                    : "dfs_count_kernel<4>";
#define SDNR_COUNT(N_, H_)                                                                   \
    do {                                                                                     \
        auto k = dfs_count_kernel<N_, H_>;                                                   \
        allow_full_lds(k);                                                                   \
        hipLaunchKernelGGL(k, dim3(cgrid), dim3(N_ * 64), cl, ctx->stream, V, ctx->adj16,    \
                           ctx->radj16, ctx->deg32, ctx->row_ptr, ctx->port, d_src, nsrc,     \
                           d_parent, d_port, d_hops);                                        \
    } while (0)
        if (nw == 2) {
            if (hops) SDNR_COUNT(2, true); else SDNR_COUNT(2, false);
        } else if (nw == 6) {
            if (hops) SDNR_COUNT(6, true); else SDNR_COUNT(6, false);
        } else {
            if (hops) SDNR_COUNT(4, true); else SDNR_COUNT(4, false);
        }
#undef SDNR_COUNT
    } else if (coop) {
        const size_t cl = dfs_lds_bytes_coop(V);
        size_t cpc = SDNR_LDS_PER_CU / cl;
        if (cpc > 8) cpc = 8;
        if (cpc < 1) cpc = 1;
        int cgrid = (int)((size_t)ctx->num_cus * cpc);
        if (cgrid > nsrc) cgrid = nsrc;
        const int kw = dfs_coop_kw();
        ctx->last_kernel = "dfs_coop_kernel";
        if (hops) launch_coop<true>(kw, cgrid, cl, ctx->stream, V, ctx->adj16, a);
        else launch_coop<false>(kw, cgrid, cl, ctx->stream, V, ctx->adj16, a);
    } else if (!small && ell && ctx->W <= 32 && packed_ok()) {
        // lanes per row = next power of two >= W
        const int lpr = ctx->W <= 8 ? 8 : (ctx->W <= 16 ? 16 : 32);
        const int ring = packed_ring(V, ctx->W);
        const size_t plds = dfs_lds_bytes_global(V, ring);
        size_t pbpc = SDNR_LDS_PER_CU / plds;
        if (pbpc > 32) pbpc = 32;                // 32 one-wave blocks fill a CU
        if (pbpc < 1) pbpc = 1;
        int pgrid = (int)((size_t)ctx->num_cus * pbpc);
        if (pgrid > nsrc) pgrid = nsrc;
        if (pgrid > grid) {                      // spill area: V entries per block
            int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes,
                                  (size_t)pgrid * (size_t)V * sizeof(uint2));
            if (rc) return rc;
            spill = static_cast<uint2 *>(ctx->scratch);
        }
        ctx->last_kernel = ring == 128 ? "dfs_global_packed_kernel<ring128>"
                                       : "dfs_global_packed_kernel";
#define SDNR_PACKED(L_, J_, H_, R_)                                                          \
    do {                                                                                     \
        auto k = dfs_global_packed_kernel<L_, J_, H_, R_>;                                   \
        allow_full_lds(k);                                                                   \
        hipLaunchKernelGGL(k, dim3(pgrid), dim3(64), plds, ctx->stream, V, ctx->W,           \
                           ctx->ell_col, ctx->ell_port, d_src, nsrc, d_parent, d_port,       \
                           d_hops, spill);                                                   \
    } while (0)
#define SDNR_PACKED_R(L_, J_, H_)                                                            \
    do {                                                                                     \
        if (ring == 128) SDNR_PACKED(L_, J_, H_, 128); else SDNR_PACKED(L_, J_, H_, 1024);   \
    } while (0)
        if (lpr == 8 && packed_j8(V) == 1) {
            if (hops) SDNR_PACKED_R(8, 1, true); else SDNR_PACKED_R(8, 1, false);
        } else if (lpr == 8) {
            if (hops) SDNR_PACKED_R(8, 2, true); else SDNR_PACKED_R(8, 2, false);
        } else if (lpr == 16) {
            if (hops) SDNR_PACKED_R(16, 4, true); else SDNR_PACKED_R(16, 4, false);
        } else {
            if (hops) SDNR_PACKED_R(32, 8, true); else SDNR_PACKED_R(32, 8, false);
        }
#undef SDNR_PACKED_R
#undef SDNR_PACKED
    } else if (narrow) {
        const int K = dfs_batch_depth(ctx);
        ctx->last_kernel = small ? "dfs_lds_batch_kernel" : "dfs_global_batch_kernel";
        if (ell && hops) launch_batch_k<true, true>(K, small, grid, lds, ctx->stream, a);
        else if (ell) launch_batch_k<true, false>(K, small, grid, lds, ctx->stream, a);
        else if (hops) launch_batch_k<false, true>(K, small, grid, lds, ctx->stream, a);
        else launch_batch_k<false, false>(K, small, grid, lds, ctx->stream, a);
    } else {
        ctx->last_kernel = small ? "dfs_lds_wide_kernel" : "dfs_global_wide_kernel";
        if (hops) launch_wide<true>(small, grid, lds, ctx->stream, a);
        else launch_wide<false>(small, grid, lds, ctx->stream, a);
    }
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}

// ---------------------------------------------------------------------------
// Twin fold.  Two switches with the same out-row and the
// same in-row, neither in the other's row (ctx->twin_rep, capi.hip), have the
// same DFS row up to 2 + |row| entries: the searches run step for step alike
// with the two in exchanged roles, the other twin only ever an inert stack
// entry (all its out-neighbours are marked by the root's pop).  A batch
// searches the first member of every class it holds (the leader) into a
// scratch table set and derives every caller row from its leader's:
//   prep    leaders, compacted to the front of a source list, their count,
//           and every position's leader row and leader
//   search  the unchanged dispatch over that list: dfs_async_kernel reads the
//           count and searches the leaders only; for any other strategy the
//           list is padded with -1 (empty rows)
//   derive  row copy + the 2 + |row| patched entries, in the layout's encoding
// ---------------------------------------------------------------------------
constexpr int kFoldPrepThreads = 1024;
constexpr int kFoldDeriveThreads = 256;
constexpr int kFoldLdsMaxV = 8000;                       // two int tables of V entries in 64 KB
constexpr int kFoldPrepListMax = 2 * kFoldPrepThreads;   // two positions per thread
constexpr size_t kFoldLdsBytes = 64 * 1024 - 256;        // dynamic LDS of the prep kernel
constexpr size_t kFoldScratchBytes = (size_t)1 << 30;    // above this the batch is not folded

// one workgroup.  Two tables indexed by class (twin_rep): first = the lowest
// batch position of the class in this batch, slot = its row in the compacted
// list; in LDS (lds != 0: V <= kFoldLdsMaxV, the whole table initialised
// while the sources load) or in global memory (only the entries this batch
// touches are initialised).  The leaders keep their batch order in csrc[0 ..
// count), the rest of csrc is -1 when pad is set (else left as it is: the
// search honours the count); lead[i] = leader row of position i (-1: src[i]
// is no vertex), lsrc[i] = that leader's source
//
// lds == 2 (the tables and the list fit LDS, nsrc <= kFoldPrepListMax): every
// thread keeps its two positions (2 tid, 2 tid + 1) and their classes in
// registers from one load of src and rep, the sources also go to LDS, and the
// compaction is one scan over both -- four LDS phases behind two dependent
// global loads, where the general path below re-reads src and rep in every
// phase and gathers lsrc from global memory
__global__ __launch_bounds__(kFoldPrepThreads) void dfs_fold_prep_kernel(
    int V, int nsrc, int lds, int pad, const int32_t *__restrict__ src,
    const int32_t *__restrict__ rep, int32_t *gtab, int32_t *__restrict__ csrc,
    int32_t *__restrict__ lead, int32_t *__restrict__ lsrc, int32_t *__restrict__ count)
{
    constexpr int NWV = kFoldPrepThreads / SDNR_WAVE;
    constexpr int kNone = 0x7FFFFFFF;
    extern __shared__ __attribute__((aligned(16))) int32_t fold_tab[];
    __shared__ int wsum[NWV];
    int32_t *first = lds ? fold_tab : gtab;
    int32_t *slot = first + V;
    const int tid = (int)threadIdx.x, lane = lane_id(), w = tid >> 6;
    if (lds == 2) {
        int32_t *ssrc = slot + V;                // the list, in LDS
        const int i0 = 2 * tid, i1 = i0 + 1;
        const int s0 = i0 < nsrc ? src[i0] : -1, s1 = i1 < nsrc ? src[i1] : -1;
        const bool ok0 = s0 >= 0 && s0 < V, ok1 = s1 >= 0 && s1 < V;
        const int r0 = ok0 ? rep[s0] : -1, r1 = ok1 ? rep[s1] : -1;
        for (int v = tid; v < V; v += kFoldPrepThreads) first[v] = kNone;
        if (i0 < nsrc) ssrc[i0] = s0;
        if (i1 < nsrc) ssrc[i1] = s1;
        __syncthreads();
        if (ok0) atomicMin(&first[r0], i0);
        if (ok1) atomicMin(&first[r1], i1);
        __syncthreads();
        const int f0 = ok0 ? first[r0] : -1, f1 = ok1 ? first[r1] : -1;
        const bool l0 = ok0 && f0 == i0, l1 = ok1 && f1 == i1;
        const uint64_t m0 = __ballot(l0), m1 = __ballot(l1);
        if (lane == 0) wsum[w] = __popcll(m0) + __popcll(m1);
        __syncthreads();
        int off = 0, total = 0;
        for (int k = 0; k < NWV; ++k) {
            const int c = wsum[k];
            if (k < w) off += c;
            total += c;
        }
        const int p0 = off + lanes_below(m0) + lanes_below(m1), p1 = p0 + (l0 ? 1 : 0);
        if (l0) {
            csrc[p0] = s0;
            slot[r0] = p0;
        }
        if (l1) {
            csrc[p1] = s1;
            slot[r1] = p1;
        }
        __syncthreads();
        if (i0 < nsrc) {
            lead[i0] = ok0 ? slot[r0] : -1;
            lsrc[i0] = ok0 ? ssrc[f0] : -1;
            if (pad && i0 >= total) csrc[i0] = -1;
        }
        if (i1 < nsrc) {
            lead[i1] = ok1 ? slot[r1] : -1;
            lsrc[i1] = ok1 ? ssrc[f1] : -1;
            if (pad && i1 >= total) csrc[i1] = -1;
        }
        if (tid == 0) count[0] = total;
        return;
    }
    if (lds) {
        for (int v = tid; v < V; v += kFoldPrepThreads) first[v] = kNone;
    } else {
        for (int i = tid; i < nsrc; i += kFoldPrepThreads) {
            const int s = src[i];
            if (s >= 0 && s < V) first[rep[s]] = kNone;
        }
    }
    __syncthreads();
    for (int i = tid; i < nsrc; i += kFoldPrepThreads) {
        const int s = src[i];
        if (s >= 0 && s < V) atomicMin(&first[rep[s]], i);
    }
    __syncthreads();
    int base = 0;                                // leaders before this chunk
    for (int i0 = 0; i0 < nsrc; i0 += kFoldPrepThreads) {
        const int i = i0 + tid;
        int s = -1, r = -1;
        if (i < nsrc) {
            s = src[i];
            if (s >= 0 && s < V) r = rep[s];
        }
        const bool leader = r >= 0 && first[r] == i;
        const uint64_t m = __ballot(leader);
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        int off = base, total = base;
        for (int k = 0; k < NWV; ++k) {
            const int c = wsum[k];
            if (k < w) off += c;
            total += c;
        }
        if (leader) {
            const int pos = off + lanes_below(m);
            csrc[pos] = s;
            slot[r] = pos;
        }
        base = total;
        __syncthreads();                         // wsum is rewritten by the next chunk
    }
    for (int i = tid; i < nsrc; i += kFoldPrepThreads) {
        const int s = src[i];
        int L = -1, ls = -1;
        if (s >= 0 && s < V) {
            const int r = rep[s];
            L = slot[r];
            ls = src[first[r]];
        }
        lead[i] = L;
        lsrc[i] = ls;
        if (pad && i >= base) csrc[i] = -1;
    }
    if (tid == 0) count[0] = base;
}

constexpr int kFoldPatchCap = kFoldDeriveThreads + 4;    // a chunk of a row's patch list, + ls
static_assert(kFoldDeriveThreads % SDNR_WAVE == 0 &&
              (kFoldDeriveThreads & (kFoldDeriveThreads - 1)) == 0, "owner rule: x >> shift & (threads - 1)");

// patch stores overlap the 16-byte copy stores of the same wave
typedef uint32_t __attribute__((may_alias)) fold_u32;
typedef uint16_t __attribute__((may_alias)) fold_u16;

// a barrier on LDS alone: no wait for the global stores in flight
__device__ __forceinline__ void fold_lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// the value is in its registers here: the compiler moves its load no further
__device__ __forceinline__ void fold_pin(uint4 &v)
{
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
}
__device__ __forceinline__ void fold_pin(uint32_t &v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void fold_pin(uint16_t &v)
{
    uint32_t x = v;
    asm volatile("" : "+v"(x));
    v = (uint16_t)x;
}

// the derive kernel's stores, copy and patch stores alike, are write-through
// (sc1): the row leaves the XCD's L2 for memory while the kernel still issues
// stores, and the end-of-dispatch release finds no 13 MB of dirty lines to
// write back before the next call's prep may start ("The
// derive kernel's store policy"; plain, nt and sc0 sc1 stores measured there).
// One policy for both kinds: a patch has to land behind the copy store of its
// word by the wave's issue order alone
typedef uint32_t __attribute__((ext_vector_type(4))) fold_v4;

__device__ __forceinline__ void fold_store(uint4 *p, const uint4 &v)
{
    const fold_v4 w = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(w) : "memory");
}
__device__ __forceinline__ void fold_store(fold_u32 *p, uint32_t v)
{
    asm volatile("global_store_dword %0, %1, off sc1" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void fold_store(fold_u16 *p, uint16_t v)
{
    asm volatile("global_store_short %0, %1, off sc1" : : "v"(p), "v"((uint32_t)v) : "memory");
}

// a row of n elements at out, a copy of the row at in (nullptr: every element
// `ones`, an empty row in every layout): element k by thread k % threads
template <typename T>
__device__ __forceinline__ void fold_copy_elems(const T *__restrict__ in, T *__restrict__ out,
                                                size_t n, T ones)
{
    constexpr size_t nt = kFoldDeriveThreads;
    if (!in) {
        for (size_t k = threadIdx.x; k < n; k += nt) fold_store(&out[k], ones);
        return;
    }
    for (size_t k0 = threadIdx.x; k0 < n; k0 += 4 * nt) {    // four loads in flight
        const size_t k1 = k0 + nt, k2 = k1 + nt, k3 = k2 + nt;
        T v0 = in[k0], v1 = in[k1 < n ? k1 : k0], v2 = in[k2 < n ? k2 : k0],
          v3 = in[k3 < n ? k3 : k0];
        // every load is issued, and has landed, before the first store: a
        // load left behind a store (sunk into its branch), or pending behind
        // a skipped one, is waited for with a count that the stores in flight
        // have to reach too
        fold_pin(v0);
        fold_pin(v1);
        fold_pin(v2);
        fold_pin(v3);
        fold_store(&out[k0], v0);
        if (k1 < n) fold_store(&out[k1], v1);
        if (k2 < n) fold_store(&out[k2], v2);
        if (k3 < n) fold_store(&out[k3], v3);
    }
}

// a row of `bytes` bytes: 16 bytes per thread and step when vec (row size and
// both tables 16-byte aligned), else in elements of es (2 or 4) bytes
__device__ __forceinline__ void fold_copy_row(const char *__restrict__ in, char *__restrict__ out,
                                              size_t bytes, int es, bool vec)
{
    if (vec)
        fold_copy_elems(reinterpret_cast<const uint4 *>(in), reinterpret_cast<uint4 *>(out),
                        bytes / 16, make_uint4(~0u, ~0u, ~0u, ~0u));
    else if (es == 4)
        fold_copy_elems(reinterpret_cast<const uint32_t *>(in), reinterpret_cast<uint32_t *>(out),
                        bytes / 4, ~0u);
    else
        fold_copy_elems(reinterpret_cast<const uint16_t *>(in), reinterpret_cast<uint16_t *>(out),
                        bytes / 2, (uint16_t)0xFFFF);
}

// one patched entry in the layout's encoding (par < 0: unreached): the words
// of table 0, table 1 (int32 layout) and the depth plane
__device__ __forceinline__ void fold_encode(int fmt, int hbytes, int par, int prt, int slot,
                                            int hop, uint32_t *w0, uint32_t *w1, uint32_t *wh)
{
    if (fmt == kTreeInt32) *w1 = (uint32_t)(par < 0 ? -1 : prt);
    if (fmt == kTreeInt32) *w0 = (uint32_t)par;
    else if (par < 0) *w0 = 0xFFFFFFFFu;
    else if (fmt == kTreePort16) *w0 = ((uint32_t)par & 0xFFFFu) | ((uint32_t)prt << 16);
    else *w0 = (uint32_t)par | ((uint32_t)slot << 26);
    if (hbytes) *wh = (uint32_t)(par < 0 ? -1 : hop);
}

// the lanes of a wave hold one patch each (column x, -1: none; word wv): the
// patches whose words this wave copied -- thread x >> shift & (threads - 1)
// is one of its -- go out in one store, after the wave's copy stores.  Two
// entries with one column in a store (parallel links in row(s)) leave it to
// the hardware which lane's word stays, as one store per thread always did
template <typename T>
__device__ __forceinline__ void fold_apply(int x, uint32_t wv, int shift, T *row)
{
    const int w = (int)threadIdx.x / SDNR_WAVE;
    if (x >= 0 && ((x >> shift) & (kFoldDeriveThreads - 1)) / SDNR_WAVE == w)
        fold_store(&row[x], (T)wv);
}

// one workgroup per caller row i: the leader's row, then -- for a row that is
// not its leader's own -- the patched entries.  With ls the leader's source
// and s this row's:
//   v in row(s)  parent s, the port / slot of s's link to v, hops 1
//   v == s       the root
//   v == ls      what the leader's row holds for s, the port / slot that of
//                the same parent's link to ls (it exists: equal in-rows)
// kFoldDeriveThreads threads copy and load nothing but lead / src / lsrc and
// the leader's row; one wave more, the patch wave, works the patches out
// meanwhile (a lane per entry of row(s), and per entry of the parent's row in
// the search for ls) and hands them over in LDS, a list of (column, encoded
// words) and its length.  After a barrier on LDS alone every patch is stored
// by the copy wave one of whose threads' stores covered its word, after that
// store: a wave's stores to one address take effect in issue order, so
// nothing waits for the copy stores' acknowledgement (by the owning thread
// alone, one store instruction a patch, the partial writes of one cache line
// queue behind each other: DESIGN.md 4.1e).  A row with more than
// kFoldDeriveThreads patches takes its list in chunks.
// fmt: table 0 is int32 parents (table 1 the ports), parent | port << 16, or
// parent | slot << 26; hbytes: 0 (no hop table), 2 or 4; vec: bit k set when
// table k (2: hops) takes the 16-byte copy
__global__ __launch_bounds__(kFoldDeriveThreads + SDNR_WAVE) void dfs_fold_derive_kernel(
    int V, int fmt, int hbytes, int vec, const int32_t *__restrict__ src,
    const int32_t *__restrict__ lsrc, const int32_t *__restrict__ lead,
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ port, const uint32_t *__restrict__ in0,
    uint32_t *__restrict__ out0, const uint32_t *__restrict__ in1, uint32_t *__restrict__ out1,
    const char *__restrict__ inh, char *__restrict__ outh, const int32_t *__restrict__ count,
    unsigned long long *pub, uint32_t seq)
{
    constexpr int nt = kFoldDeriveThreads;
    __shared__ int32_t p_col[kFoldPatchCap];     // the patch list: column (-1: none),
    __shared__ uint32_t p_w0[kFoldPatchCap];     // the word of every table,
    __shared__ uint32_t p_w1[kFoldPatchCap];
    __shared__ uint32_t p_wh[kFoldPatchCap];
    __shared__ int32_t p_d;                      // and |row(s)|
    const size_t i = blockIdx.x;
    const int tid = (int)threadIdx.x, lane = lane_id();
    const bool patcher = uniform(tid / SDNR_WAVE) == nt / SDNR_WAVE;
    // pub (a coherent host word, may be null): the live count of this call
    // for the host's choice of the next call's search form, one 8-byte store
    // by one thread; its acknowledgement is waited for under the copy
    const bool tell = pub && i == 0 && tid == 0;
    const uint32_t searched = tell ? (uint32_t)count[0] : 0u;
    const int L = uniform(lead[i]), s = uniform(src[i]), ls = uniform(lsrc[i]);
    if (tell)
        __hip_atomic_store(pub, (unsigned long long)seq << 32 | searched, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    const bool patch = L >= 0 && s != ls;        // else an empty row, or the leader's as it is
    const size_t ob = i * (size_t)V, lb = (size_t)(L < 0 ? 0 : L) * (size_t)V;
    // the patch wave and the copy waves meet at barriers of their own, so
    // that neither's waits are merged into the other's path (patcher is
    // wave-uniform, and a scalar branch)
    if (patcher) {
        if (!patch) return;
        // first trip: what the leader's row holds for s, and row(s)'s bounds
        const uint32_t e = in0[lb + s];
        int hop = -1;
        if (hbytes == 2) hop = reinterpret_cast<const uint16_t *>(inh)[lb + s];
        else if (hbytes == 4) hop = reinterpret_cast<const int32_t *>(inh)[lb + s];
        const int a = uniform(row_ptr[s]), d = uniform(row_ptr[s + 1]) - a;
        if (lane == 0) p_d = d;
        // chunk c0 of the list: entry t - c0 is that of row(s)[t], of the root
        // for t == d
        auto entries = [&](int c0, int first) {
            for (int k = first; k < nt && c0 + k <= d; k += SDNR_WAVE) {
                const int t = c0 + k;
                p_col[k] = t < d ? col[a + t] : s;
                fold_encode(fmt, hbytes, s, t < d ? port[a + t] : -1, t < d ? t : 63,
                            t < d ? 1 : 0, &p_w0[k], &p_w1[k], &p_wh[k]);
            }
        };
        // second trip: row(s), a lane per entry, and the parent's row bounds
        int av = -1, aprt = -1;
        if (lane < d) {
            av = col[a + lane];
            aprt = port[a + lane];
        }
        const int par = fmt == kTreeInt32 ? (int)e
                        : e == 0xFFFFFFFFu ? -1
                        : (int)(e & (fmt == kTreePort16 ? 0xFFFFu : 0x3FFFFFFu));
        int lo = 0, n = 0;
        if (par >= 0) {
            lo = row_ptr[par];
            n = row_ptr[par + 1] - lo;
        }
        // third trip: the parent's row, a lane per entry
        int cv = -1, cprt = -1;
        if (lane < n) {
            cv = col[lo + lane];
            cprt = port[lo + lane];
        }
        if (lane <= d) {
            p_col[lane] = lane < d ? av : s;
            fold_encode(fmt, hbytes, s, aprt, lane < d ? lane : 63, lane < d ? 1 : 0, &p_w0[lane],
                        &p_w1[lane], &p_wh[lane]);
        }
        entries(0, lane + SDNR_WAVE);            // what a lane per entry has not covered
        // the entry of ls comes last in the first chunk, written by the lane
        // that found it (none: no entry)
        int bv = -1, bpar = -1, bprt = -1, bslot = 63, bhop = -1;
        if (par < 0) {
            if (lane == 0) bv = ls;
        } else {
            if (lane < n && cv == ls) {
                bv = ls;
                bpar = par;
                bprt = cprt;
                bslot = lane;
                bhop = hop;
            }
            for (int k = lane + SDNR_WAVE; k < n; k += SDNR_WAVE)
                if (col[lo + k] == ls) {
                    bv = ls;
                    bpar = par;
                    bprt = port[lo + k];
                    bslot = k;
                    bhop = hop;
                }
        }
        const int nb = d < nt ? d + 1 : nt;
        const uint64_t fm = __ballot(bv >= 0);
        if (lane == (fm ? __ffsll((unsigned long long)fm) - 1 : 0)) {
            p_col[nb] = bv;
            fold_encode(fmt, hbytes, bpar, bprt, bslot, bhop, &p_w0[nb], &p_w1[nb], &p_wh[nb]);
        }
        fold_lds_barrier();                      // the list is complete
        for (int c0 = nt; c0 <= d; c0 += nt) {   // a row wider than the workgroup
            fold_lds_barrier();                  // the owners are done with the last chunk
            entries(c0, lane);
            fold_lds_barrier();
        }
        return;
    }
    fold_copy_row(L < 0 ? nullptr : reinterpret_cast<const char *>(in0 + lb),
                  reinterpret_cast<char *>(out0 + ob), 4 * (size_t)V, 4, (vec & 1) != 0);
    if (fmt == kTreeInt32)
        fold_copy_row(L < 0 ? nullptr : reinterpret_cast<const char *>(in1 + lb),
                      reinterpret_cast<char *>(out1 + ob), 4 * (size_t)V, 4, (vec & 2) != 0);
    if (hbytes)
        fold_copy_row(L < 0 ? nullptr : inh + lb * hbytes, outh + ob * hbytes,
                      (size_t)hbytes * V, hbytes, (vec & 4) != 0);
    if (!patch) return;
    // the patch stores below follow this wave's copy stores in issue order,
    // whichever of its lanes stores: wavefront scope, no instruction
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    // the owner of a word by its table's copy form
    const int sh0 = (vec & 1) ? 2 : 0, sh1 = (vec & 2) ? 2 : 0,
              shh = (vec & 4) ? (hbytes == 2 ? 3 : 2) : 0;
    fold_lds_barrier();
    const int d = uniform(p_d);
    for (int c0 = 0; c0 <= d; c0 += nt) {
        if (c0) {
            fold_lds_barrier();
            fold_lds_barrier();
        }
        const int left = d + 1 - c0;
        const int nent = (left < nt ? left : nt) + (c0 ? 0 : 1);
        for (int e0 = 0; e0 < nent; e0 += SDNR_WAVE) {
            const int k = e0 + lane;
            const int x = k < nent ? p_col[k] : -1;
            fold_apply(x, k < nent ? p_w0[k] : 0u, sh0, reinterpret_cast<fold_u32 *>(out0 + ob));
            if (fmt == kTreeInt32)
                fold_apply(x, k < nent ? p_w1[k] : 0u, sh1, reinterpret_cast<fold_u32 *>(out1 + ob));
            if (hbytes == 2)
                fold_apply(x, k < nent ? p_wh[k] : 0u, shh, reinterpret_cast<fold_u16 *>(outh) + ob);
            else if (hbytes == 4)
                fold_apply(x, k < nent ? p_wh[k] : 0u, shh, reinterpret_cast<fold_u32 *>(outh) + ob);
        }
    }
}

// the parts of the trimmed fold (A/B builds: -DSDNR_FOLD_PARTS=n leaves some
// out): 1 the search honours the live count, 4 the prep kernel's short form
#ifndef SDNR_FOLD_PARTS
#define SDNR_FOLD_PARTS 5
#endif

// the dispatch honours a live count for this call: dfs_async_kernel, run
// directly (the slot layout goes through int32 tables and a pack pass over
// every row, which then must all be defined)
static bool dfs_takes_live(const sdnr_ctx *ctx, int nsrc, bool hops, bool packed, bool slots)
{
    return dfs_async(ctx, nsrc, hops) && !(packed && slots);
}

// fold this batch?  Only a graph with twins, and by default only above 2
// sources per CU, the boundary dfs_async_waves uses.  Up to
// it the batch size itself selects the 8-wave kernel and the fold only adds
// its two launches (forced on, k=48 144 / 288 sources lose 6.6 / 0.8 us);
// above it the folded search runs 8 waves from its second call on, the
// unfolded one 4: 516 / 576 / 640 sources 52.9 / 53.4 / 53.6 us folded, 63.6 /
// 65.0 / 65.1 not (profiles/fold_waves_ab.txt; with the folded search at 4
// waves 516 and 576 tied, and the constant was 2.5).  SDNROUTE_DFS_FOLD=0|1
// forces it off / on (A/B, tests on tiny batches)
static bool dfs_fold(const sdnr_ctx *ctx, int nsrc)
{
    if (!ctx->has_twins) return false;
    if (const char *f = getenv("SDNROUTE_DFS_FOLD")) {
        if (!strcmp(f, "0")) return false;
        if (!strcmp(f, "1")) return true;
    }
    return (int64_t)nsrc > 2 * (int64_t)ctx->num_cus;
}

// live searches per CU up to which the folded search takes its low-load form:
// the boundary dfs_async_waves uses.  No crossover was found above it -- k=48,
// 1,152 sources of which 48 / 256 / 512 / 1,152 are classes of their own, us
// per call (median), full form 67.4 / 133.2 / 138.4 / 171.0, low form 62.9 /
// 103.3 / 108.9 / 152.6 -- so above 2 per CU the full form
// stays for what it is everywhere else, the choice of the unfolded path at
// this load, until that path's own rows are measured again
constexpr int kFoldLowPerCu = 2;

// the folded search in its low-load form?  SDNROUTE_DFS_FOLD_FORM=full|low
// forces either (A/B, tests).  *count: the published count the answer was
// taken from, 0 where it was forced
static bool dfs_fold_low(sdnr_ctx *ctx, int nsrc, int32_t *count)
{
    *count = 0;
    if (const char *f = getenv("SDNROUTE_DFS_FOLD_FORM")) {
        if (!strcmp(f, "full")) return false;
        if (!strcmp(f, "low")) return true;
    }
    // the count the derive kernel of an earlier folded call published: read
    // once, never waited for.  It counts only when its sequence number is a
    // launch of this graph upload with this nsrc (live_ring); a stale or
    // missing one only picks a slower one of several bit-exact kernels --
    // the search itself reads the count from the device
    const unsigned long long w = __atomic_load_n(ctx->h_live, __ATOMIC_RELAXED);
    const uint32_t seq = (uint32_t)(w >> 32);
    if (seq == 0) return false;
    for (const auto &r : ctx->live_ring)
        if (r.seq0 && seq - r.seq0 <= r.seq1 - r.seq0) {     // the run that launch was in
            if (r.gen != ctx->upload_gen || r.nsrc != nsrc ||
                (int64_t)(uint32_t)w > (int64_t)kFoldLowPerCu * ctx->num_cus)
                return false;
            *count = (int32_t)(uint32_t)w;
            return true;
        }
    return false;
}

int sdnr_launch_dfs(sdnr_ctx *ctx, const int32_t *d_src, int32_t nsrc,
                    int32_t *d_parent, int32_t *d_port, int32_t *d_hops, uint32_t *d_tree,
                    bool slots, bool hops16)
{
    const int V = ctx->V;
    ctx->dfs_nsrc = nsrc;
    ctx->dfs_folded = false;
    ctx->dfs_form = kDfsFormFull;
    ctx->dfs_quotient = false;
    if (nsrc == 0 || V == 0 || !dfs_fold(ctx, nsrc))
        return dfs_dispatch(ctx, d_src, nsrc, d_parent, d_port, d_hops, d_tree, slots, hops16);
    const bool packed = d_tree != nullptr;
    const size_t n = (size_t)nsrc * (size_t)V;
    const int hbytes = d_hops ? (hops16 ? 2 : 4) : 0;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // scratch3: the searched count, the compacted sources, every position's
    // leader row and leader, the prep kernel's two class tables, then the
    // leaders' table set in the caller's layout
    const size_t o_csrc = 256, o_lead = o_csrc + up(4 * (size_t)nsrc),
                 o_lsrc = o_lead + up(4 * (size_t)nsrc), o_tab = o_lsrc + up(4 * (size_t)nsrc),
                 o_t0 = o_tab + up(8 * (size_t)V), o_t1 = o_t0 + up(4 * n),
                 o_h = o_t1 + (packed ? 0 : up(4 * n)), need = o_h + up((size_t)hbytes * n);
    if (need > kFoldScratchBytes)
        return dfs_dispatch(ctx, d_src, nsrc, d_parent, d_port, d_hops, d_tree, slots, hops16);
    int rc = sdnr_reserve(&ctx->scratch3, &ctx->scratch3_bytes, need);
    if (rc) return rc;
    char *sb = static_cast<char *>(ctx->scratch3);
    int32_t *count = reinterpret_cast<int32_t *>(sb);
    int32_t *csrc = reinterpret_cast<int32_t *>(sb + o_csrc);
    int32_t *lead = reinterpret_cast<int32_t *>(sb + o_lead);
    int32_t *lsrc = reinterpret_cast<int32_t *>(sb + o_lsrc);
    int32_t *tab = reinterpret_cast<int32_t *>(sb + o_tab);
    int32_t *t0 = reinterpret_cast<int32_t *>(sb + o_t0);
    int32_t *t1 = packed ? nullptr : reinterpret_cast<int32_t *>(sb + o_t1);
    int32_t *th = hbytes ? reinterpret_cast<int32_t *>(sb + o_h) : nullptr;
    // SDNROUTE_DFS_FOLD_LDS=0 keeps the class tables in global memory (tests)
    const char *fl = getenv("SDNROUTE_DFS_FOLD_LDS");
    const bool lds = V <= kFoldLdsMaxV && !(fl && !strcmp(fl, "0"));
    // the prep kernel's short form: the tables and the list in LDS
    const bool lds2 = lds && (SDNR_FOLD_PARTS & 4) && nsrc <= kFoldPrepListMax &&
                      8 * (size_t)V + 4 * (size_t)nsrc <= kFoldLdsBytes;
    // a strategy that honours the live count searches the leaders only; any
    // other gets the list padded with -1, so that its rows stay defined
    const bool live = (SDNR_FOLD_PARTS & 1) && dfs_takes_live(ctx, nsrc, hbytes != 0, packed, slots);
    int32_t live_n = 0;                          // the published count, where the form is its choice
    const bool low = live && dfs_fold_low(ctx, nsrc, &live_n);
    uint32_t seq = 0;                            // this launch in the ring of published counts
    if (live) {
        if (!(seq = ++ctx->live_seq)) seq = ++ctx->live_seq;
        auto *r = &ctx->live_ring[ctx->live_head];
        if (r->seq0 && r->seq1 + 1 == seq && r->gen == ctx->upload_gen && r->nsrc == nsrc) {
            r->seq1 = seq;                       // one more of the same run
        } else {
            ctx->live_head = (ctx->live_head + 1) % kLiveRing;
            r = &ctx->live_ring[ctx->live_head];
            r->seq0 = r->seq1 = seq;
            r->gen = ctx->upload_gen;
            r->nsrc = nsrc;
        }
    }
    const bool timed = ctx->timed;
    if (timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(dfs_fold_prep_kernel, dim3(1), dim3(kFoldPrepThreads),
                       lds2 ? 8 * (size_t)V + 4 * (size_t)nsrc : (lds ? 8 * (size_t)V : 0),
                       ctx->stream, V, nsrc, lds2 ? 2 : (lds ? 1 : 0), live ? 0 : 1, d_src,
                       ctx->twin_rep, tab, csrc, lead, lsrc, count);
    SDNR_HIP(hipGetLastError());
    ctx->timed = false;                          // the span is timed around the three launches
    rc = dfs_dispatch(ctx, csrc, nsrc, packed ? nullptr : t0, t1, th,
                      packed ? reinterpret_cast<uint32_t *>(t0) : nullptr, slots, hops16,
                      live ? count : nullptr, low, live_n);
    ctx->timed = timed;
    if (rc) return rc;
    uint32_t *o0 = packed ? d_tree : reinterpret_cast<uint32_t *>(d_parent);
    auto vec_ok = [&](const void *p, size_t row_bytes) {
        return row_bytes % 16 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0;
    };
    const int vec = (vec_ok(o0, 4 * (size_t)V) ? 1 : 0) |
                    (!packed && vec_ok(d_port, 4 * (size_t)V) ? 2 : 0) |
                    (hbytes && vec_ok(d_hops, (size_t)hbytes * V) ? 4 : 0);
    const int fmt = packed ? (slots ? kTreeSlot : kTreePort16) : kTreeInt32;
    hipLaunchKernelGGL(dfs_fold_derive_kernel, dim3(nsrc), dim3(kFoldDeriveThreads + SDNR_WAVE), 0,
                       ctx->stream, V, fmt, hbytes, vec, d_src, lsrc, lead, ctx->row_ptr,
                       ctx->col, ctx->port, reinterpret_cast<const uint32_t *>(t0), o0,
                       reinterpret_cast<const uint32_t *>(t1), reinterpret_cast<uint32_t *>(d_port),
                       reinterpret_cast<const char *>(th), reinterpret_cast<char *>(d_hops), count,
                       live ? ctx->h_live : nullptr, seq);
    SDNR_HIP(hipGetLastError());
    ctx->dfs_folded = true;
    ctx->last_launches = 3;                      // prep, search, derive
    if (timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}
