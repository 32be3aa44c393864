// remote_lfa.hip -- remote loop-free alternates (RFC 7490): a PQ-node repair
// tunnel per directed link.
//
// With D(a, b) = P[b][a] the least cost a -> b (P the caller's all-pairs
// table, row v = destination v) and a link e = (S -> E) of cost c, E != S:
//   Q-space           X != S, D(X,E) finite and
//                     (D(X,S) INF or D(X,E) < D(X,S) + c)
//   extended P-space  through an out-neighbour N of S, N != E, N != S:
//                     D(N,X) finite and (D(N,S) INF or D(E,X) INF or
//                     D(N,X) < D(N,S) + c + D(E,X))
// -- no least-cost route X -> E, N -> X uses e.  The repair of e is the pair
// (X, N) in both of the smallest key (cost(S -> N) + D(N,X), X, N): tunnel to
// X through N.  Everything is integer; three table entries may sum to
// 3 (2^32 - 2), so the sums are u64, and INF enters none.
//
// D(N, .) and D(E, .) are columns of P.  A pre-pass transposes P into the
// context scratch (PT[a][x] = D(a, x); tiled through LDS, both sides
// coalesced), after which everything the main kernel streams is a contiguous
// row: PT[N_j][.], P[E_i][.], P[S][.].
//
// Main kernel: one workgroup per source vertex S, persistent over the units.
// The links of S go in passes of 64, and what belongs to a link alone -- its
// head N_j, its cost and D(N_j,S) = P[S][N_j] -- is read once per pass, lane l
// for link 64 * pass + l, and fetched by a lane read where a loop needs it.  A
// wavefront takes 64 consecutive X, lane l the vertex 64 * blk + l, and first
// reads D(N_j, X) of every slot of the row, keeping the first kRlfaTile of
// them in LDS -- a column of the tile belongs to one lane, so the tile needs no
// barrier; the slots past the tile are read again from L2 where they are
// needed: the tile is small because workgroups per CU are worth more than LDS
// hits here (16 slots, eight workgroups per CU: 2.9 ms on the k=48 fat-tree;
// the whole row, three per CU: 4.5 ms; no tile 3.3 ms) -- and takes
// lb(X) = min_j cost_j + D(N_j,X), a lower bound of every key at X.  A key is
// tunnel cost << 28 | X << 14 | slot (cost < 2^34, X and slot < 2^14, slots
// ascend with N), one u64 per link of the pass in LDS.  The block's smallest
// (lb(X), X, 0) is voted against those 64 keys: the links it cannot improve
// are skipped for the whole block.  The Q test of the others is one u64 of bits
// per lane (independent row loads), and a link runs the O(deg) selection at X
// only where its Q bit is set and (lb(X), X, 0) is still below its best key.
// The lanes' keys are reduced by shuffles, then one LDS atomicMin per
// wavefront.  The pass ends with one thread per link decoding its key and
// writing the link's five entries.
#include "common.h"

namespace {

constexpr int kRlfaThreads = 256;
constexpr int kRlfaWaves = kRlfaThreads / SDNR_WAVE;
constexpr int kRlfaPass = SDNR_WAVE;               // links per pass: one per lane, their Q bits one u64
constexpr int kRlfaTile = 16;                      // slots of D(N_j, X) a wavefront stages at most
constexpr int kTrTile = 64;                        // the transpose's tile edge
constexpr uint32_t kRlfaInf = SDNR_COST_INF;
constexpr unsigned long long kNoKey = ~0ull;
// sdnr_graph_upload takes strictly ascending rows only: a vertex has no two
// links to one head, so a row has at most V slots and slot i is the only one
// whose head is E_i (the selection's N != E is j != i)
static_assert(kLfaMaxV <= 1 << 14, "a key holds X and the slot in 14 bits each");

// PT[a][x] = P[x][a]
__global__ __launch_bounds__(256) void remote_lfa_transpose_kernel(
    int V, const uint32_t *__restrict__ p, uint32_t *__restrict__ pt)
{
    __shared__ uint32_t t[kTrTile][kTrTile + 1];
    const int tx = (int)threadIdx.x & 63, ty = (int)threadIdx.x >> 6;
    const int bx = (int)blockIdx.x * kTrTile, by = (int)blockIdx.y * kTrTile;
    for (int r = ty; r < kTrTile; r += 4)
        if (by + r < V && bx + tx < V)
            t[r][tx] = p[(size_t)(by + r) * (size_t)V + (size_t)(bx + tx)];
    __syncthreads();
    for (int r = ty; r < kTrTile; r += 4)
        if (bx + r < V && by + tx < V)
            pt[(size_t)(bx + r) * (size_t)V + (size_t)(by + tx)] = t[tx][r];
}

// 64 links of S's row, one per lane: the head, D(head, S) and the cost; a
// lane past the row holds S itself, which every loop skips
struct RlfaLinks {
    int n;
    uint32_t back, cost;
};

__device__ __forceinline__ RlfaLinks rlfa_links(int lo, int deg, int jb, int lane, int S,
                                                const int32_t *__restrict__ col,
                                                const uint32_t *__restrict__ cost,
                                                const uint32_t *__restrict__ ps)
{
    RlfaLinks g{S, 0u, 1u};
    const int j = jb + lane;
    if (j < deg) {
        g.n = col[lo + j];
        g.back = ps[g.n];
        if (cost) g.cost = cost[lo + j];
    }
    return g;
}

// PRUNE: skip the selection where lb(X) cannot beat the link's best key (the
// alternative measured: every Q-space vertex runs it)
template <bool PRUNE>
__global__ __launch_bounds__(kRlfaThreads) void remote_lfa_kernel(
    int V, int nverts, int tslots, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const int32_t *__restrict__ port,
    const uint32_t *__restrict__ cost, const uint32_t *__restrict__ pall,
    const uint32_t *__restrict__ pt, const int32_t *__restrict__ verts, int32_t *__restrict__ pq,
    int32_t *__restrict__ via, int32_t *__restrict__ via_port,
    unsigned long long *__restrict__ tunnel_cost, uint8_t *__restrict__ kind,
    uint32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t rlfa_tile[];   // [waves][tslots][64]
    __shared__ unsigned long long best[kRlfaPass];
    __shared__ uint32_t cnt[4];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t *tile = rlfa_tile + (size_t)wave * (size_t)tslots * SDNR_WAVE + lane;
    const int nblk = (V + SDNR_WAVE - 1) / SDNR_WAVE;

    for (int u = (int)blockIdx.x; u < nverts; u += (int)gridDim.x) {
        const int sv = verts ? verts[u] : u;
        if (sv < 0 || sv >= V) {                           // an empty unit
            if (counts && tid < 4) counts[(size_t)u * 4 + tid] = 0;
            continue;
        }
        const int S = sv;
        const int lo = row_ptr[S], deg = row_ptr[S + 1] - lo;
        const uint32_t *ps = pall + (size_t)S * (size_t)V;             // ps[x] = D(x, S)
        if (tid < 4) cnt[tid] = 0;
        for (int base = 0; base < deg; base += kRlfaPass) {
            const int n = deg - base < kRlfaPass ? deg - base : kRlfaPass;
            const RlfaLinks mine_l = rlfa_links(lo, deg, base, lane, S, col, cost, ps);
            if (tid < kRlfaPass) best[tid] = kNoKey;
            __syncthreads();
            for (int blk = wave; blk < nblk; blk += kRlfaWaves) {
                const int X = blk * SDNR_WAVE + lane;
                const bool valid = X < V && X != S;
                const size_t xc = (size_t)(X < V ? X : V - 1);         // the column every load takes
                // the tile column of X and the lower bound of its keys
                unsigned long long lb = kNoKey;
                for (int jb = 0; jb < deg; jb += SDNR_WAVE) {
                    const RlfaLinks g = jb == base ? mine_l
                                                   : rlfa_links(lo, deg, jb, lane, S, col, cost, ps);
                    const int m = deg - jb < SDNR_WAVE ? deg - jb : SDNR_WAVE;
                    for (int jj = 0; jj < m; ++jj) {
                        const int nj = read_lane(g.n, jj);
                        const uint32_t cj = (uint32_t)read_lane((int)g.cost, jj);
                        const uint32_t d = pt[(size_t)nj * (size_t)V + xc];
                        if (jb + jj < tslots) tile[(size_t)(jb + jj) * SDNR_WAVE] = d;
                        const unsigned long long tc = (unsigned long long)cj + d;
                        if (nj != S && d != kRlfaInf && tc < lb) lb = tc;
                    }
                }
                const unsigned long long xkey = (unsigned long long)(X & 0x3FFF) << 14;
                const unsigned long long lbkey =
                    !valid || lb == kNoKey ? kNoKey : (lb << 28 | xkey);
                // the links of the pass this block can still improve: lane l
                // votes for link l with the block's smallest bound
                unsigned long long live = n < 64 ? (1ull << n) - 1 : kNoKey;
                if (PRUNE) {
                    unsigned long long low = lbkey;
#pragma unroll
                    for (int w = SDNR_WAVE / 2; w > 0; w >>= 1) {
                        const unsigned long long o = __shfl_xor(low, w);
                        low = o < low ? o : low;
                    }
                    live &= __ballot(low < __hip_atomic_load(&best[lane], __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_WORKGROUP));
                }
                if (!live) continue;
                // the Q bits of those links
                const uint32_t dxs = ps[xc];
                unsigned long long qm = 0;
                for (unsigned long long left = live; left; left &= left - 1) {
                    const int ii = __builtin_ctzll(left);
                    const int ei = read_lane(mine_l.n, ii);
                    const uint32_t ci = (uint32_t)read_lane((int)mine_l.cost, ii);
                    const uint32_t dxe = pall[(size_t)ei * (size_t)V + xc];
                    const bool q = ei != S && dxe != kRlfaInf &&
                                   (dxs == kRlfaInf ||
                                    (unsigned long long)dxe < (unsigned long long)dxs + ci);
                    qm |= (unsigned long long)(q ? 1 : 0) << ii;
                }
                if (lbkey == kNoKey) qm = 0;               // no vertex here, or none reaches it
                for (unsigned long long left = live; left; left &= left - 1) {
                    const int ii = __builtin_ctzll(left);
                    bool act = ((qm >> ii) & 1) != 0;
                    if (!__any(act)) continue;
                    const unsigned long long cur = __hip_atomic_load(
                        &best[ii], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (PRUNE) {
                        act = act && lbkey < cur;
                        if (!__any(act)) continue;
                    }
                    const int i = base + ii;
                    const int ei = read_lane(mine_l.n, ii);
                    const unsigned long long ci = (uint32_t)read_lane((int)mine_l.cost, ii);
                    const uint32_t dex = i < tslots ? tile[(size_t)i * SDNR_WAVE]
                                                    : pt[(size_t)ei * (size_t)V + xc];
                    unsigned long long mine = kNoKey;
                    for (int jb = 0; jb < deg; jb += SDNR_WAVE) {
                        const RlfaLinks g = jb == base
                                                ? mine_l
                                                : rlfa_links(lo, deg, jb, lane, S, col, cost, ps);
                        const int m = deg - jb < SDNR_WAVE ? deg - jb : SDNR_WAVE;
                        for (int jj = 0; jj < m; ++jj) {
                            const int j = jb + jj;
                            const int nj = read_lane(g.n, jj);
                            if (j == i || nj == S) continue;
                            const uint32_t bj = (uint32_t)read_lane((int)g.back, jj);   // D(N_j, S)
                            const uint32_t cj = (uint32_t)read_lane((int)g.cost, jj);
                            const uint32_t d = j < tslots ? tile[(size_t)j * SDNR_WAVE]
                                                          : pt[(size_t)nj * (size_t)V + xc];
                            const bool in_p =
                                d != kRlfaInf &&
                                (bj == kRlfaInf || dex == kRlfaInf ||
                                 (unsigned long long)d < (unsigned long long)bj + ci + dex);
                            const unsigned long long key =
                                ((unsigned long long)cj + d) << 28 | xkey | (unsigned long long)j;
                            if (act && in_p && key < mine) mine = key;
                        }
                    }
#pragma unroll
                    for (int w = SDNR_WAVE / 2; w > 0; w >>= 1) {
                        const unsigned long long o = __shfl_xor(mine, w);
                        mine = o < mine ? o : mine;
                    }
                    if (lane == 0 && mine < cur) atomicMin(&best[ii], mine);
                }
            }
            __syncthreads();
            // one thread per link of the pass (wave 0, lane = link): decode
            // the key, write the five entries
            bool linked = false, rep = false, plain = false, lfa = false;
            if (tid < n) {
                const int e = lo + base + tid;
                const int ei = mine_l.n;
                const unsigned long long key = best[tid];
                int x = -1, nv = -1, np = -1;
                unsigned long long tc = 0;
                linked = ei != S;
                if (key != kNoKey) {
                    const int slot = (int)(key & 0x3FFF);
                    x = (int)(key >> 14 & 0x3FFF);
                    tc = key >> 28;
                    nv = col[lo + slot];
                    np = port[lo + slot];
                    const uint32_t dsx = pt[(size_t)S * (size_t)V + (size_t)x];
                    const uint32_t dex = pt[(size_t)ei * (size_t)V + (size_t)x];
                    rep = true;
                    plain = dsx != kRlfaInf &&
                            (dex == kRlfaInf ||
                             (unsigned long long)dsx < (unsigned long long)mine_l.cost + dex);
                    lfa = x == nv;
                }
                pq[e] = x;
                via[e] = nv;
                via_port[e] = np;
                tunnel_cost[e] = tc;
                kind[e] = (uint8_t)((rep ? 1u : 0u) | (plain ? 2u : 0u) | (lfa ? 4u : 0u));
            }
            if (wave == 0) {                               // the pass's links are wave 0's lanes
                const uint32_t c0 = (uint32_t)__popcll(__ballot(linked));
                const uint32_t c1 = (uint32_t)__popcll(__ballot(rep));
                const uint32_t c2 = (uint32_t)__popcll(__ballot(plain));
                const uint32_t c3 = (uint32_t)__popcll(__ballot(lfa));
                if (lane == 0) {
                    cnt[0] += c0;
                    cnt[1] += c1;
                    cnt[2] += c2;
                    cnt[3] += c3;
                }
            }
            __syncthreads();                               // best[] is reused by the next pass
        }
        __syncthreads();                                   // (a vertex without links: cnt is set)
        if (counts && tid < 4) counts[(size_t)u * 4 + tid] = cnt[tid];
        __syncthreads();                                   // cnt is reused by the next unit
    }
}

template <bool PRUNE>
int launch_main(sdnr_ctx *ctx, const char *name, const uint32_t *cost, const uint32_t *d_pall,
                const uint32_t *pt, const int32_t *d_verts, int32_t nverts, int32_t *d_pq,
                int32_t *d_via, int32_t *d_via_port, uint64_t *d_tunnel_cost, uint8_t *d_kind,
                uint32_t *d_counts)
{
    // the tile: the first kRlfaTile slots of the rows
    int tile = kRlfaTile;
    // the measured alternatives (diagnostic build only): SDNROUTE_RLFA_TILE=n,
    // a tile of n <= 64 slots (0: every D(N_j, X) read from L2), and
    // SDNROUTE_RLFA_PER_CU=n, at most n workgroups per CU
    const char *ts = sdnr_tune_env("SDNROUTE_RLFA_TILE");
    if (ts && atoi(ts) >= 0 && atoi(ts) <= 64) tile = atoi(ts);
    const int tslots = ctx->max_deg < tile ? ctx->max_deg : tile;
    const size_t lds = (size_t)kRlfaWaves * (size_t)tslots * SDNR_WAVE * sizeof(uint32_t);
    auto fn = remote_lfa_kernel<PRUNE>;
    sdnr_allow_lds(reinterpret_cast<const void *>(fn), lds);
    // workgroups per CU: what the tiles leave of the LDS, at most 2048 threads
    int per_cu = 2048 / kRlfaThreads;
    if (lds * (size_t)per_cu > SDNR_LDS_PER_CU - 1024)
        per_cu = (int)((SDNR_LDS_PER_CU - 1024) / lds);
    const char *pc = sdnr_tune_env("SDNROUTE_RLFA_PER_CU");
    if (pc && atoi(pc) >= 1 && atoi(pc) < per_cu) per_cu = atoi(pc);
    int64_t g = (int64_t)ctx->num_cus * per_cu;
    if (g > nverts) g = nverts;
    ctx->last_kernel = name;
    ctx->last_launches = 1;
    ctx->last_grid = g;
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(kRlfaThreads), lds, ctx->stream, ctx->V, nverts,
                       tslots, ctx->row_ptr, ctx->col, ctx->port, cost, d_pall, pt, d_verts, d_pq,
                       d_via, d_via_port, reinterpret_cast<unsigned long long *>(d_tunnel_cost),
                       d_kind, d_counts);
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    return SDNR_OK;
}

}  // namespace

int sdnr_launch_remote_lfa(sdnr_ctx *ctx, const uint32_t *d_pall, const int32_t *d_verts,
                           int32_t nverts, int32_t *d_pq, int32_t *d_via, int32_t *d_via_port,
                           uint64_t *d_tunnel_cost, uint8_t *d_kind, uint32_t *d_counts)
{
    const int V = ctx->V;
    const uint32_t *cost = ctx->has_cost ? ctx->cost : nullptr;    // none: every link costs 1
    const size_t pt_bytes = (size_t)V * (size_t)V * sizeof(uint32_t);
    if (pt_bytes > kLoadsScratchBytes)
        return sdnr_fail(SDNR_ERR_NOMEM, "sdnr_remote_lfa: the transposed all-pairs table takes "
                         "%zu bytes, above the %zu of scratch", pt_bytes, kLoadsScratchBytes);
    const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, pt_bytes);
    if (rc) return rc;
    uint32_t *pt = static_cast<uint32_t *>(ctx->scratch);
    const unsigned tg = (unsigned)((V + kTrTile - 1) / kTrTile);
    hipLaunchKernelGGL(remote_lfa_transpose_kernel, dim3(tg, tg), dim3(256), 0, ctx->stream, V,
                       d_pall, pt);
    SDNR_HIP(hipGetLastError());
#ifdef SDNR_DIAG_VARIANTS
    // the measured alternative (diagnostic build only, SDNROUTE_RLFA_NOPRUNE=1)
    const char *f = sdnr_tune_env("SDNROUTE_RLFA_NOPRUNE");
    if (f && f[0] == '1')
        return launch_main<false>(ctx, "remote_lfa_kernel<noprune>", cost, d_pall, pt, d_verts,
                                  nverts, d_pq, d_via, d_via_port, d_tunnel_cost, d_kind, d_counts);
#endif
    return launch_main<true>(ctx, "remote_lfa_kernel", cost, d_pall, pt, d_verts, nverts, d_pq,
                             d_via, d_via_port, d_tunnel_cost, d_kind, d_counts);
}
