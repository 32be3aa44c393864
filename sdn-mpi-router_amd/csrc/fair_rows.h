// fair_rows.h -- the row pass and the entry step of progressive filling, shared
// by fair_rates.hip (one filling, the host passes the round) and fair_times.hip
// (a filling per epoch, the round and the epoch come from device memory).  The
// definition and the shape of the two kernels are stated in fair_rates.hip;
// what fair_times.hip adds is marked TIMES here and compiles away without it.
// The constants, FairTimes, the clock and the TIMES helpers that the multipath
// forms (ecmp_fair_rows.h) share are in fair_epochs.h.
#ifndef SDNR_FAIR_ROWS_H
#define SDNR_FAIR_ROWS_H

#include "fair_epochs.h"

namespace {

constexpr int kFairThreads = 512;
constexpr int kFairLinkThreads = 256;

struct FairRows {
    const uint32_t *tree;     // [nrows][V]: int32 parents / next hops, port16 or slot words
    int layout;               // SDNR_TREE_INT32 / SDNR_TREE_PORT16 / SDNR_TREE_SLOT
    int to_root;              // rows are next-hop rows: the link is v -> parent
};

struct FairState {
    unsigned long long *n;        // [E + nextra] counts of the running round (zero between rounds)
    unsigned long long *n_prev;   // [E + nextra] counts of the round before
    double *rem;                  // [E + nextra] capacity left
    double *share;                // [E + nextra] rem / n of the last link pass
    double *used;                 // [E + nextra] the caller's
    unsigned long long *level;    // [max_rounds + 1] bits of r_k, +inf until round k ran
    long long *alive_row;         // [nrows] alive flows of a row
    unsigned long long *status;   // 0: running, k + 1: r_k was +inf
    unsigned int *ticket;         // workgroups of the running link pass that are done
};

// what the tree word of v says: its parent (kFairNone: none), and whether v is
// a root of the row (its own parent, or -- in next-hop rows, which hold -1 at
// the destination -- without a next hop)
constexpr int kFairNone = -1, kFairBadWord = -2;

__device__ __forceinline__ int fair_parent(const FairRows &t, size_t rb, int v, int V, int *slot,
                                           bool *root)
{
    const uint32_t w = t.tree[rb + v];
    int p;
    *slot = -1;
    *root = false;
    if (t.layout == SDNR_TREE_PORT16) {
        p = (int)(w & 0xFFFFu);
        if (p == 0xFFFF) return kFairNone;
    } else if (t.layout == SDNR_TREE_SLOT) {
        if (w == 0xFFFFFFFFu) return kFairNone;
        p = (int)(w & 0x3FFFFFFu);
        *slot = (int)(w >> 26);
    } else {
        p = (int)w;
        if (p < 0) {
            *root = t.to_root != 0;
            return kFairNone;
        }
    }
    if (p == v) {
        *root = true;
        return kFairNone;
    }
    if (p >= V) return kFairBadWord;
    return p;
}

// index of the CSR entry (u, x), -1 if u has no such link
__device__ __forceinline__ int fair_edge_index(const int32_t *__restrict__ row_ptr,
                                               const int32_t *__restrict__ col, int u, int x)
{
    int lo = row_ptr[u], hi = row_ptr[u + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return (lo < row_ptr[u + 1] && col[lo] == x) ? lo : -1;
}

// an extra constraint's index, -1 for none or for one outside [E, E + nextra)
__device__ __forceinline__ int fair_extra(const int32_t *__restrict__ extra, int64_t i, int j,
                                          int E, int nextra)
{
    if (!extra) return -1;
    const int x = extra[2 * i + j];
    return (x >= E && (int64_t)x < (int64_t)E + nextra) ? x : -1;
}

// a subtree sum: in global scratch the adds are L2 atomics, so the reads go there too
template <bool LDS>
__device__ __forceinline__ unsigned long long fair_sum(const unsigned long long *p)
{
    return LDS ? *p : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The row pass of round k over the rows r = blockIdx.x, + gridDim.x, ...: the
// verdict of round k - 1 (k == 0: the flows' classification; TIMES in a later
// epoch: the advance by dt) and the counts of round k.
// JT: u16 (LDS, none 0xFFFF) or u32 (global scratch, none 0xFFFFFFFF)
template <typename JT, bool LDS, bool TIMES>
__device__ __forceinline__ void fair_rows_body(
    const FairRows &t, int V, int E, int nextra, int nrows, int max_steps, int k,
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int64_t *__restrict__ pair_off, int64_t pair_lo, int64_t pair_hi,
    const int32_t *__restrict__ verts, const uint64_t *__restrict__ mult,
    const int32_t *__restrict__ extra, const FairState &s, double *__restrict__ rate,
    int32_t *__restrict__ bott, int32_t *__restrict__ round, unsigned char *__restrict__ scratch,
    size_t scratch_stride, int *__restrict__ err, int errbit, const FairTimes &ft,
    unsigned long long *fair_lds, unsigned long long *s_alive)
{
    constexpr JT kNone = (JT)~(JT)0;
    const double r_prev =
        k > 0 ? __longlong_as_double((long long)s.level[k - 1]) : 0.0;
    const double inf = __longlong_as_double((long long)kInfBits);
    // generation g of the sums / ancestors: A0 + g * V, J0 + g * V; B aliases A
    unsigned long long *A0;
    if (LDS)
        A0 = fair_lds;
    else
        A0 = reinterpret_cast<unsigned long long *>(scratch + (size_t)blockIdx.x * scratch_stride);
    JT *J0 = reinterpret_cast<JT *>(A0 + 2 * (size_t)V);
    int *Ev = reinterpret_cast<int *>(J0 + 2 * (size_t)V);
    int *B0 = reinterpret_cast<int *>(A0);
    const int tid = (int)threadIdx.x;

    for (int r = (int)blockIdx.x; r < nrows; r += (int)gridDim.x) {
        const int64_t lo = pair_off[r], hi = pair_off[r + 1];
        if (lo < pair_lo || hi > pair_hi || hi < lo) {     // offsets outside the pair list
            if (tid == 0) atomicOr(err, errbit);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no flow)
        if (k > 0 && s.alive_row[r] == 0) continue;        // (uniform: none of them alive)
        if (TIMES && k == 0 && ft.j > 0 && ft.inflight_row[r] == 0) continue;  // (none in flight)
        const size_t rb = (size_t)r * (size_t)V;
        bool bad = false;

        // J_0 = parent, e_v = the link of v toward the root
        int any0 = 0;
        for (int v = tid; v < V; v += kFairThreads) {
            int slot;
            bool root;
            int p = fair_parent(t, rb, v, V, &slot, &root);
            int e = -1;
            if (p == kFairBadWord) {
                bad = true;
                p = kFairNone;
            }
            if (p >= 0) {
                if (t.to_root) {
                    e = fair_edge_index(row_ptr, col, v, p);
                } else if (t.layout == SDNR_TREE_SLOT) {
                    e = row_ptr[p] + slot;
                    if (e >= row_ptr[p + 1] || col[e] != v) e = -1;
                } else {
                    e = fair_edge_index(row_ptr, col, p, v);
                }
                if (e < 0 || e >= E) {                     // a tree link the graph does not have
                    bad = true;
                    e = -1;
                }
            }
            J0[v] = p < 0 ? kNone : (JT)p;
            Ev[v] = e;
            any0 |= p >= 0;
        }
        if (tid == 0) *s_alive = 0;
        const int more0 = __syncthreads_or(any0);

        unsigned long long mine = 0;                       // this thread's flows still alive
        if (k == 0 && (!TIMES || ft.j == 0)) {
            // classify the row's flows (rate 0.0, bott -1, round -1 are preset;
            // TIMES: time +inf, epoch -1, rate0 0.0, remaining = bytes)
            for (int64_t i = lo + tid; i < hi; i += kFairThreads) {
                const int x = verts[i];
                if (x < 0 || x >= V) continue;
                if (mult && mult[i] == 0) continue;        // absent
                int slot;
                bool root;
                const int p = fair_parent(t, rb, x, V, &slot, &root);
                if (p < 0 && !root) continue;              // unreached in this row
                if (extra) {
                    const int x0 = extra[2 * i], x1 = extra[2 * i + 1];
                    if ((x0 != -1 && fair_extra(extra, i, 0, E, nextra) < 0) ||
                        (x1 != -1 && fair_extra(extra, i, 1, E, nextra) < 0))
                        atomicOr(err, errbit);             // (that constraint is ignored)
                }
                double nb = 0.0;
                if (TIMES) {
                    nb = ft.bytes[i];
                    if (!(nb >= 0.0) || nb == inf) continue;   // absent (the start pass reports it)
                }
                if (p < 0 && fair_extra(extra, i, 0, E, nextra) < 0 &&
                    fair_extra(extra, i, 1, E, nextra) < 0) {
                    if (TIMES) {
                        ft.rate0[i] = inf;
                        ft.time[i] = 0.0;
                        ft.remaining[i] = 0.0;
                    } else {
                        rate[i] = inf;                     // no link and no extra
                    }
                    continue;
                }
                if (TIMES && nb == 0.0) {                  // nothing to send: never shares
                    ft.time[i] = 0.0;
                    continue;
                }
                round[i] = kFairAlive;
                if (TIMES && ft.max_epochs == 0) ft.epoch[i] = -2;
                ++mine;
            }
        } else if (TIMES && k == 0) {
            // the advance of epoch j - 1: a flow that sent its bytes leaves, the
            // others go into this epoch's filling with what they have left
            for (int64_t i = lo + tid; i < hi; i += kFairThreads) {
                const int rd = round[i];
                if (rd == -1) continue;
                if (rd == kFairAlive) {                    // never frozen (a bad capacity): out
                    round[i] = -1;
                    continue;
                }
                const double b = ft.remaining[i], ri = rate[i];
                const double left = fair_bytes_left(b, ri, ft.dt);
                if (b / ri == ft.dt || left <= 0.0) {
                    ft.time[i] = ft.t;
                    ft.epoch[i] = ft.j - 1;
                    ft.remaining[i] = 0.0;
                    round[i] = -1;
                } else {
                    ft.remaining[i] = left;
                    round[i] = kFairAlive;
                    if (ft.j == ft.max_epochs) ft.epoch[i] = -2;
                    ++mine;
                }
            }
        } else {
            // (a) the verdict of round k - 1: first saturated link toward the root
            for (int v = tid; v < V; v += kFairThreads) {
                const int e = Ev[v];
                B0[v] = (e >= 0 && s.share[e] == r_prev) ? e : -1;
            }
            __syncthreads();
            int cur = 0, steps = 0, more = more0;
            while (more && steps < max_steps) {
                const int *Bc = B0 + (cur ? V : 0);
                int *Bn = B0 + (cur ? 0 : V);
                const JT *Jc = J0 + (cur ? V : 0);
                JT *Jn = J0 + (cur ? 0 : V);
                int any = 0;
                for (int v = tid; v < V; v += kFairThreads) {
                    const JT j = Jc[v];
                    int b = Bc[v];
                    JT jj = kNone;
                    if (j != kNone) {
                        if (b < 0) b = Bc[j];
                        jj = Jc[j];
                        any |= jj != kNone;
                    }
                    Bn[v] = b;
                    Jn[v] = jj;
                }
                more = __syncthreads_or(any);
                cur ^= 1;
                ++steps;
            }
            const int *B = B0 + (cur ? V : 0);
            for (int64_t i = lo + tid; i < hi; i += kFairThreads) {
                if (round[i] != kFairAlive) continue;
                int b = B[verts[i]];
                if (b < 0) {
                    const int x0 = fair_extra(extra, i, 0, E, nextra);
                    const int x1 = fair_extra(extra, i, 1, E, nextra);
                    if (x0 >= 0 && s.share[x0] == r_prev) b = x0;
                    else if (x1 >= 0 && s.share[x1] == r_prev) b = x1;
                }
                if (b >= 0) {
                    rate[i] = r_prev;
                    if (TIMES) {
                        if (ft.j == 0) ft.rate0[i] = r_prev;
                    } else {
                        bott[i] = b;
                    }
                    round[i] = k - 1;
                } else {
                    ++mine;
                }
            }
        }
        if (mine) atomicAdd(s_alive, mine);
        __syncthreads();                                   // (B is read; A may be filled)
        const unsigned long long alive = *s_alive;
        if (tid == 0) {
            s.alive_row[r] = (long long)alive;
            if (TIMES && k == 0) ft.inflight_row[r] = (long long)alive;
        }
        // (bad is per thread; the row is dropped by all or none.  Only round 0
        // can find a bad row: later rounds skip it)
        int badrow = k == 0 ? __syncthreads_or(bad ? 1 : 0) : 0;
        int cur = 0;
        if (!badrow && alive) {
            // (b) A_0 = alive multiplicity, J_0 = parent again
            for (int v = tid; v < V; v += kFairThreads) {
                A0[v] = 0;
                if (k > 0) {
                    int slot;
                    bool root;
                    const int p = fair_parent(t, rb, v, V, &slot, &root);
                    J0[v] = p < 0 ? kNone : (JT)p;
                }
            }
            __syncthreads();
            for (int64_t i = lo + tid; i < hi; i += kFairThreads) {
                if (round[i] != kFairAlive) continue;
                const unsigned long long w = mult ? (unsigned long long)mult[i] : 1ull;
                atomicAdd(&A0[verts[i]], w);
            }
            __syncthreads();

            int steps = 0, more = more0;
            while (more) {
                if (steps == max_steps) {                      // an ancestor chain longer than V
                    bad = true;
                    break;
                }
                unsigned long long *Ac = A0 + (cur ? V : 0), *An = A0 + (cur ? 0 : V);
                JT *Jc = J0 + (cur ? V : 0), *Jn = J0 + (cur ? 0 : V);
                for (int v = tid; v < V; v += kFairThreads)
                    An[v] = fair_sum<LDS>(&Ac[v]);
                __syncthreads();
                int any = 0;
                for (int v = tid; v < V; v += kFairThreads) {
                    const JT j = Jc[v];
                    JT jj = kNone;
                    if (j != kNone) {
                        const unsigned long long a = fair_sum<LDS>(&Ac[v]);
                        if (a) atomicAdd(&An[j], a);
                        jj = Jc[j];
                        any |= jj != kNone;
                    }
                    Jn[v] = jj;
                }
                more = __syncthreads_or(any);
                cur ^= 1;
                ++steps;
            }
            badrow = __syncthreads_or(bad ? 1 : 0);
        }
        if (badrow) {
            // its flows stay 0.0 / -1 / -1 (TIMES: absent, whatever they were)
            for (int64_t i = lo + tid; i < hi; i += kFairThreads) {
                if (TIMES) {
                    round[i] = -1;
                    ft.time[i] = inf;
                    ft.epoch[i] = -1;
                    ft.rate0[i] = 0.0;
                    ft.remaining[i] = ft.bytes[i];
                } else if (round[i] == kFairAlive) {
                    round[i] = -1;
                }
            }
            if (tid == 0) {
                atomicOr(err, errbit);
                s.alive_row[r] = 0;
                if (TIMES) ft.inflight_row[r] = 0;
            }
            __syncthreads();                               // s_alive is reset by the next row
            continue;
        }
        if (alive == 0) {
            __syncthreads();
            continue;
        }

        // n[e_v] += T[v], n[extra] += mult
        const unsigned long long *T = A0 + (cur ? V : 0);
        for (int v = tid; v < V; v += kFairThreads) {
            const unsigned long long x = fair_sum<LDS>(&T[v]);
            const int e = Ev[v];
            if (x && e >= 0) atomicAdd(&s.n[e], x);
        }
        if (extra) {
            for (int64_t i = lo + tid; i < hi; i += kFairThreads) {
                if (round[i] != kFairAlive) continue;
                const unsigned long long w = mult ? (unsigned long long)mult[i] : 1ull;
                const int x0 = fair_extra(extra, i, 0, E, nextra);
                const int x1 = fair_extra(extra, i, 1, E, nextra);
                if (x0 >= 0) atomicAdd(&s.n[x0], w);
                if (x1 >= 0 && x1 != x0) atomicAdd(&s.n[x1], w);
            }
        }
        __syncthreads();                                   // the buffers are reused by the next row
    }
}

// The entry step of round k over the E + nextra entries: step 2, share,
// n_prev = n, n = 0 and a wave-reduced minimum into level[k] (atomicMin on the
// bits: non-negative doubles order as their bit patterns).
__device__ __forceinline__ void fair_links_step(const FairState &s, int n_ent, int k)
{
    // the multiply, the add and the subtract of step 2 round one by one, as the
    // host's numpy does: no fused multiply-add (HIP contracts by default, and
    // the __d*_rn intrinsics are plain operators that contract all the same)
#pragma clang fp contract(off)
    const double inf = __longlong_as_double((long long)kInfBits);
    const int e = (int)(blockIdx.x * (unsigned)kFairLinkThreads + threadIdx.x);
    double sh = inf;
    if (e < n_ent) {
        const unsigned long long cnt = s.n[e];
        double rem = s.rem[e];
        if (k > 0) {
            const unsigned long long m = s.n_prev[e] - cnt;
            if (m) {
                const double r_prev = __longlong_as_double((long long)s.level[k - 1]);
                const double p = r_prev * (double)m;
                s.used[e] = s.used[e] + p;
                rem = fmax(rem - p, 0.0);
                s.rem[e] = rem;
            }
        }
        if (cnt) sh = rem / (double)cnt;
        s.share[e] = sh;
        s.n_prev[e] = cnt;
        s.n[e] = 0;
    }
    // rem >= 0 and cnt > 0: sh is a non-negative double or +inf, ordered as its bits
    unsigned long long bits = (unsigned long long)__double_as_longlong(sh);
    for (int d = SDNR_WAVE / 2; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(bits, d, SDNR_WAVE);
        bits = o < bits ? o : bits;
    }
    if (lane_id() == 0 && bits != kInfBits) atomicMin(&s.level[k], bits);
}

// The shape of the row kernel for a graph of V vertices and nrows rows: its
// form, dynamic LDS, per-workgroup scratch stride and grid.
struct FairShape {
    bool lds_form;
    size_t lds, stride;
    int64_t grid;
    int max_steps;            // ceil(log2 V) + 1
};

inline FairShape fair_shape(const sdnr_ctx *ctx, int nrows)
{
    const int V = ctx->V;
    FairShape f;
    f.max_steps = 1;
    while ((1ll << (f.max_steps - 1)) < (long long)V) ++f.max_steps;
    f.lds_form = V <= kFairLdsMaxV;
    f.lds = f.lds_form ? (size_t)V * kFairBytesPerV : 0;
    f.stride = f.lds_form ? 0 : ((((size_t)V * 28) + 255) & ~(size_t)255);
    int64_t g;
    if (f.lds_form) {
        int per_cu = (int)(SDNR_LDS_PER_CU / (f.lds ? f.lds : 1));
        per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);     // 2048 threads per CU
        g = (int64_t)ctx->num_cus * per_cu;
    } else {
        g = ctx->num_cus;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / f.stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
    }
    if (g > nrows) g = nrows;
    f.grid = g;
    return f;
}

}  // namespace

#endif  // SDNR_FAIR_ROWS_H
