// ecmp_fair_rows.h -- the row pass and the link step of progressive filling
// over ECMP, shared by ecmp_fair_rates.hip (one filling, the host passes the
// round) and ecmp_fair_times.hip (a filling per epoch, the round and the epoch
// come from device memory).  The definition and the shape of the two kernels
// are stated in ecmp_fair_rates.hip; what ecmp_fair_times.hip adds is marked
// TIMES here and compiles away without it.
#ifndef SDNR_ECMP_FAIR_ROWS_H
#define SDNR_ECMP_FAIR_ROWS_H

#include "fair_epochs.h"

namespace {

constexpr int kEcmpFairThreads = 1024;   // chains of dependent LDS / L2 reads, as cost_ecmp_loads.hip
constexpr int kEcmpFairLinkThreads = 256;
constexpr double kFairTie = 0x1p-30;     // shares within r_k * kFairTie of r_k tie with it
constexpr uint32_t kEfInf = SDNR_COST_INF;
constexpr int kNoLink = 0x7FFFFFFF;      // B[x]: no saturated link below x

struct EcmpFairState {
    double *a;                    // [E + nextra] counts of the running round (zero between rounds)
    double *a_prev;               // [E + nextra] counts of the round before
    double *rem;                  // [E + nextra] capacity left
    double *share;                // [E + nextra] rem / a of the last link pass
    double *used;                 // [E + nextra] the caller's
    unsigned long long *level;    // [max_rounds + 1] bits of r_k, +inf until round k ran
    long long *alive_row;         // [nrows] alive flows of a row
    unsigned long long *status;   // 0: running, k + 1: r_k was +inf
    unsigned int *ticket;         // workgroups of the running link pass that are done
};

// words in scratch are written by other waves of the workgroup (plain or L2
// atomics): agent-scope accesses read past L1
template <bool LDS>
__device__ __forceinline__ double ef_ld_f64(const double *p)
{
    if (LDS) return *p;
    return __longlong_as_double((long long)__hip_atomic_load(
        reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT));
}

template <bool LDS>
__device__ __forceinline__ void ef_st_f64(double *p, double v)
{
    if (LDS)
        *p = v;
    else
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(p),
                           (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ int ef_ld_i32(const int *p)
{
    return LDS ? *p : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ void ef_st_i32(int *p, int v)
{
    if (LDS)
        *p = v;
    else
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// depth words: u16 in LDS (a depth is < V <= kEcmpFairLdsMaxV), u32 in scratch;
// kPending (above every sweep number) marks a vertex that is not final yet
template <bool LDS>
struct EfDepth;
template <>
struct EfDepth<true> {
    typedef uint16_t T;
    static constexpr int kPending = 0xFFFF;
    static __device__ __forceinline__ int ld(const T *p) { return (int)*p; }
    static __device__ __forceinline__ void st(T *p, int v) { *p = (T)v; }
};
template <>
struct EfDepth<false> {
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

// the largest share that ties with the level r: r + r * kFairTie, the multiply
// and the add rounded one by one as the host's numpy does (TIMES: the largest
// q that ends with dt, by the same rule)
__device__ __forceinline__ double ef_tie_bound(double r)
{
#pragma clang fp contract(off)
    const double t = r * kFairTie;
    return r + t;
}

// an extra constraint's index, -1 for none or for one outside [E, E + nextra)
__device__ __forceinline__ int ef_extra(const int32_t *__restrict__ extra, int64_t i, int j, int E,
                                        int nextra)
{
    if (!extra) return -1;
    const int x = extra[2 * i + j];
    return (x >= E && (int64_t)x < (int64_t)E + nextra) ? x : -1;
}

// The row pass of round k over the rows r = blockIdx.x, + gridDim.x, ...: the
// verdict of round k - 1 (k == 0: the flows' classification; TIMES in a later
// epoch: the advance by dt) and the counts of round k.
// hop: sigma[x] holds the number of next hops instead of the route count;
// cost NULL: every link costs 1.  round[] with TIMES is FairTimes' (fair_epochs.h).
// TIMES with min_q set is the advance phase instead: the minimum of q over each
// row's flows in flight, atomicMin on the bits into *min_q (k is 0 then).  It
// shares the row loop, so the kernel holds one loop over the rows, not two.
// ecmp_fair_lds, LDS form: sigma f64 [V] | flow f64 [V] | pcost u32 [V] | depth u16 [V]
template <bool LDS, bool TIMES>
__device__ __forceinline__ void ecmp_fair_rows_body(
    int V, int E, int nextra, int nrows, int hop, int k, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const uint32_t *__restrict__ cost,
    const uint32_t *__restrict__ pcost, const int64_t *__restrict__ pair_off, int64_t pair_lo,
    int64_t pair_hi, const int32_t *__restrict__ srcs, const uint64_t *__restrict__ mult,
    const int32_t *__restrict__ extra, const EcmpFairState &s, double *__restrict__ rate,
    int32_t *__restrict__ bott, int32_t *__restrict__ round, unsigned char *__restrict__ scratch,
    size_t scratch_stride, int *__restrict__ err, int errbit, const FairTimes &ft,
    unsigned long long *min_q, unsigned char *ecmp_fair_lds, unsigned long long *s_alive)
{
    typedef EfDepth<LDS> Dp;
    typedef typename Dp::T depth_t;
    const double inf = __longlong_as_double((long long)kInfBits);
    const double r_prev = k > 0 ? __longlong_as_double((long long)s.level[k - 1]) : 0.0;
    const double tie = ef_tie_bound(r_prev);
    unsigned char *base = LDS ? ecmp_fair_lds : scratch + (size_t)blockIdx.x * scratch_stride;
    double *sigma = reinterpret_cast<double *>(base);
    double *flow = sigma + V;
    int *B = reinterpret_cast<int *>(flow);                // dead before (b) seeds flow
    // LDS: flow | pcost | depth; scratch: flow | depth
    uint32_t *pc_lds = reinterpret_cast<uint32_t *>(flow + V);
    depth_t *depth = LDS ? reinterpret_cast<depth_t *>(pc_lds + V)
                         : reinterpret_cast<depth_t *>(flow + V);
    const int tid = (int)threadIdx.x;

    for (int r = (int)blockIdx.x; r < nrows; r += (int)gridDim.x) {
        const int64_t lo = pair_off[r], hi = pair_off[r + 1];
        if (lo < pair_lo || hi > pair_hi || hi < lo) {     // offsets outside the pair list
            if (tid == 0) atomicOr(err, errbit);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no flow)
        if (TIMES && min_q) {
            // dt = min q over the flows in flight (all frozen by now)
            if (ft.inflight_row[r] == 0) continue;
            unsigned long long bits = kInfBits;
            for (int64_t i = lo + tid; i < hi; i += kEcmpFairThreads) {
                if (round[i] < 0) continue;
                // rem_b > 0 and rate > 0: q is positive or +inf, ordered as its bits
                const unsigned long long b =
                    (unsigned long long)__double_as_longlong(ft.remaining[i] / rate[i]);
                bits = b < bits ? b : bits;
            }
            for (int d = SDNR_WAVE / 2; d > 0; d >>= 1) {
                const unsigned long long o = __shfl_xor(bits, d, SDNR_WAVE);
                bits = o < bits ? o : bits;
            }
            if (lane_id() == 0 && bits < kInfBits) atomicMin(min_q, bits);
            continue;
        }
        if (k > 0 && s.alive_row[r] == 0) continue;        // (uniform: none of them alive)
        if (TIMES && k == 0 && ft.j > 0 && ft.inflight_row[r] == 0) continue;  // (none in flight)
        const uint32_t *prow = pcost + (size_t)r * (size_t)V;
        const uint32_t *pc = LDS ? pc_lds : prow;

        // 1. the destination (pcost 0) and the unreachable are final at depth 0
        for (int x = tid; x < V; x += kEcmpFairThreads) {
            const uint32_t px = prow[x];
            if (LDS) pc_lds[x] = px;
            ef_st_f64<LDS>(&sigma[x], (px == 0 && !hop) ? 1.0 : 0.0);
            Dp::st(&depth[x], (px == 0 || px == kEfInf) ? 0 : Dp::kPending);
        }
        if (tid == 0) *s_alive = 0;
        __syncthreads();

        // 2. depth and sigma: sweep j finalises the vertices whose longest chain is j
        //    (hop split: sigma = the number of next hops)
        bool bad = false, done = false;
        int top = 0;
        for (int j = 1; j <= V; ++j) {
            int pending = 0;
            for (int x = tid; x < V; x += kEcmpFairThreads) {
                if (Dp::ld(&depth[x]) != Dp::kPending) continue;
                const uint32_t px = pc[x];
                double c = 0.0;
                bool any = false, ready = true;
                const int re = row_ptr[x + 1];
                for (int e = row_ptr[x]; e < re; ++e) {
                    const int n = col[e];
                    const uint32_t pn = pc[n];
                    // (64-bit sum: a row that is no labelling must not wrap into a tie)
                    if (pn == kEfInf || (uint64_t)pn + (cost ? cost[e] : 1u) != (uint64_t)px)
                        continue;
                    if (Dp::ld(&depth[n]) >= j) {          // pending, or finalised in this sweep
                        ready = false;
                        break;
                    }
                    any = true;
                    c += hop ? 1.0 : ef_ld_f64<LDS>(&sigma[n]);
                }
                if (!ready) {
                    pending = 1;
                    continue;
                }
                // no next hop (a finite pcost > 0 that no link explains), dead next hops, overflow
                if (!(c > 0.0) || c > 1.7976931348623157e308) {
                    bad = true;
                    c = 0.0;
                }
                ef_st_f64<LDS>(&sigma[x], c);
                Dp::st(&depth[x], any ? j : 0);
            }
            top = j;
            if (!__syncthreads_or(pending)) {
                done = true;
                break;
            }
        }
        if (!done) bad = true;                             // (uniform) no DAG of V vertices does that
        // (only round 0 can find a bad row: later rounds skip it.  Its flows
        // stay 0.0 / -1 / -1 -- TIMES: absent, as the start pass preset them,
        // and a later epoch finds nothing of it in flight -- and it
        // contributes nothing)
        if (k == 0 && __syncthreads_or(bad ? 1 : 0)) {
            if (tid == 0) {
                atomicOr(err, errbit);
                s.alive_row[r] = 0;
                if (TIMES) ft.inflight_row[r] = 0;
            }
            continue;
        }

        unsigned long long mine = 0;                       // this thread's flows still alive
        if (k == 0 && (!TIMES || ft.j == 0)) {
            // classify the row's flows (rate 0.0, bott -1, round -1 are preset;
            // TIMES: time +inf, epoch -1, rate0 0.0, remaining = bytes)
            for (int64_t i = lo + tid; i < hi; i += kEcmpFairThreads) {
                const int x = srcs[i];
                if (x < 0 || x >= V) continue;
                if (mult && mult[i] == 0) continue;        // absent
                const uint32_t px = pc[x];
                if (px == kEfInf) continue;                // unreachable
                if (extra) {
                    const int x0 = extra[2 * i], x1 = extra[2 * i + 1];
                    if ((x0 != -1 && ef_extra(extra, i, 0, E, nextra) < 0) ||
                        (x1 != -1 && ef_extra(extra, i, 1, E, nextra) < 0))
                        atomicOr(err, errbit);             // (that constraint is ignored)
                }
                double nb = 0.0;
                if (TIMES) {
                    nb = ft.bytes[i];
                    if (!(nb >= 0.0) || nb == inf) continue;   // absent (the start pass reports it)
                }
                if (px == 0 && ef_extra(extra, i, 0, E, nextra) < 0 &&
                    ef_extra(extra, i, 1, E, nextra) < 0) {
                    if (TIMES) {
                        ft.rate0[i] = inf;
                        ft.time[i] = 0.0;
                        ft.remaining[i] = 0.0;
                    } else {
                        rate[i] = inf;                     // s == d and no extra
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
            // the advance of epoch j - 1: a flow that sent its bytes, or is
            // within the tie tolerance of the first to do so, leaves; the others
            // go into this epoch's filling with what they have left
            const double bound = ef_tie_bound(ft.dt);
            for (int64_t i = lo + tid; i < hi; i += kEcmpFairThreads) {
                const int rd = round[i];
                if (rd == -1) continue;
                if (rd == kFairAlive) {                    // never frozen (a bad capacity): out
                    round[i] = -1;
                    continue;
                }
                const double b = ft.remaining[i], ri = rate[i];
                const double left = fair_bytes_left(b, ri, ft.dt);
                if (b / ri <= bound || left <= 0.0) {
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
            // (a) the verdict of round k - 1: the smallest saturated link below every vertex
            for (int x = tid; x < V; x += kEcmpFairThreads)
                if (Dp::ld(&depth[x]) == 0) ef_st_i32<LDS>(&B[x], kNoLink);
            __syncthreads();
            for (int D = 1; D <= top; ++D) {
                for (int x = tid; x < V; x += kEcmpFairThreads) {
                    if (Dp::ld(&depth[x]) != D) continue;
                    const uint32_t px = pc[x];
                    int b = kNoLink;
                    const int re = row_ptr[x + 1];
                    for (int e = row_ptr[x]; e < re; ++e) {
                        const int n = col[e];
                        const uint32_t pn = pc[n];
                        if (pn == kEfInf || (uint64_t)pn + (cost ? cost[e] : 1u) != (uint64_t)px)
                            continue;
                        if (e < b && s.share[e] <= tie) b = e;
                        const int bn = ef_ld_i32<LDS>(&B[n]);   // (depth[n] < D: final)
                        b = bn < b ? bn : b;
                    }
                    ef_st_i32<LDS>(&B[x], b);
                }
                __syncthreads();
            }
            for (int64_t i = lo + tid; i < hi; i += kEcmpFairThreads) {
                if (round[i] != kFairAlive) continue;
                int b = ef_ld_i32<LDS>(&B[srcs[i]]);
                if (b == kNoLink) {
                    const int x0 = ef_extra(extra, i, 0, E, nextra);
                    const int x1 = ef_extra(extra, i, 1, E, nextra);
                    if (x0 >= 0 && s.share[x0] <= tie) b = x0;
                    else if (x1 >= 0 && s.share[x1] <= tie) b = x1;
                }
                if (b != kNoLink) {
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
        __syncthreads();                                   // (B is read; flow may be seeded)
        const unsigned long long alive = *s_alive;
        if (tid == 0) {
            s.alive_row[r] = (long long)alive;
            if (TIMES && k == 0) ft.inflight_row[r] = (long long)alive;
        }
        // (TIMES, round 0 of epoch max_epochs: the call is capped after this
        // pass, which only had to apply the last advance: no counts)
        if (alive == 0 || (TIMES && k == 0 && ft.j == ft.max_epochs)) {
            __syncthreads();                               // s_alive is reset by the next row
            continue;
        }

        // (b) the counts of round k: the alive multiplicities enter at their sources
        for (int x = tid; x < V; x += kEcmpFairThreads) ef_st_f64<LDS>(&flow[x], 0.0);
        __syncthreads();
        for (int64_t i = lo + tid; i < hi; i += kEcmpFairThreads) {
            if (round[i] != kFairAlive) continue;
            const double w = (double)(mult ? mult[i] : 1ull);
            const int x = srcs[i];
            if (pc[x] != 0) atomicAdd(&flow[x], w);        // (s == d: only its extras count)
            const int x0 = ef_extra(extra, i, 0, E, nextra);
            const int x1 = ef_extra(extra, i, 1, E, nextra);
            if (x0 >= 0) atomicAdd(&s.a[x0], w);
            if (x1 >= 0 && x1 != x0) atomicAdd(&s.a[x1], w);
        }
        __syncthreads();
        // ... and are pushed down the DAG, deepest first
        for (int D = top; D >= 1; --D) {
            for (int x = tid; x < V; x += kEcmpFairThreads) {
                if (Dp::ld(&depth[x]) != D) continue;
                const double f = ef_ld_f64<LDS>(&flow[x]);
                const double sx = ef_ld_f64<LDS>(&sigma[x]);
                if (!(f > 0.0) || !(sx > 0.0)) continue;
                const uint32_t px = pc[x];
                const int re = row_ptr[x + 1];
                for (int e = row_ptr[x]; e < re; ++e) {
                    const int n = col[e];
                    const uint32_t pn = pc[n];
                    if (pn == kEfInf || (uint64_t)pn + (cost ? cost[e] : 1u) != (uint64_t)px)
                        continue;
                    // sigma[n] <= sigma[x]: the share is in [0, 1]
                    const double g = hop ? f / sx : f * (ef_ld_f64<LDS>(&sigma[n]) / sx);
                    if (!(g > 0.0)) continue;
                    if (pn != 0) atomicAdd(&flow[n], g);   // (pcost 0: the destination absorbs)
                    atomicAdd(&s.a[e], g);
                }
            }
            __syncthreads();
        }
    }
}

// The link step of round k over the E + nextra entries: step 2, share,
// a_prev = a, a = 0 and a wave-reduced minimum into level[k] (atomicMin on the
// bits: non-negative doubles order as their bit patterns).
__device__ __forceinline__ void ecmp_fair_links_step(const EcmpFairState &s, int n_ent, int k)
{
    // the subtract, the multiply, the add and the subtract of step 2 round one
    // by one, as the host's numpy does: no fused multiply-add
#pragma clang fp contract(off)
    const double inf = __longlong_as_double((long long)kInfBits);
    const int e = (int)(blockIdx.x * (unsigned)kEcmpFairLinkThreads + threadIdx.x);
    double sh = inf;
    if (e < n_ent) {
        const double cnt = s.a[e];
        double rem = s.rem[e];
        if (k > 0) {
            const double m = fmax(s.a_prev[e] - cnt, 0.0);
            if (m > 0.0) {
                const double r_prev = __longlong_as_double((long long)s.level[k - 1]);
                const double p = r_prev * m;
                s.used[e] = s.used[e] + p;
                rem = fmax(rem - p, 0.0);
                s.rem[e] = rem;
            }
        }
        if (cnt > 0.0) sh = rem / cnt;
        s.share[e] = sh;
        s.a_prev[e] = cnt;
        s.a[e] = 0.0;
    }
    // rem >= 0 and cnt > 0: sh is a non-negative double or +inf, ordered as its bits
    unsigned long long bits = (unsigned long long)__double_as_longlong(sh);
    for (int d = SDNR_WAVE / 2; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(bits, d, SDNR_WAVE);
        bits = o < bits ? o : bits;
    }
    if (lane_id() == 0 && bits != kInfBits) atomicMin(&s.level[k], bits);
}

// The last workgroup of round k's link pass closes the level: r_k = max(min
// share, r_{k-1}).  True when r_k is +inf (no link holds an alive flow).
__device__ __forceinline__ bool ecmp_fair_close_level(const EcmpFairState &s, int k)
{
    const unsigned long long lv =
        __hip_atomic_load(&s.level[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lv == kInfBits) return true;
    if (k > 0 && lv < s.level[k - 1]) s.level[k] = s.level[k - 1];
    return false;
}

// The shape of the row kernel for a graph of V vertices and nrows rows: its
// form, dynamic LDS, per-workgroup scratch stride and grid.
struct EcmpFairShape {
    bool lds_form;
    size_t lds, stride;
    int64_t grid;
};

inline EcmpFairShape ecmp_fair_shape(const sdnr_ctx *ctx, int nrows)
{
    const int V = ctx->V;
    EcmpFairShape f;
    f.lds_form = V <= kEcmpFairLdsMaxV;
    f.lds = f.lds_form ? (((size_t)V * kEcmpFairBytesPerV + 15) & ~(size_t)15) : 0;
    f.stride = f.lds_form ? 0 : ((((size_t)V * 20) + 255) & ~(size_t)255);
    int64_t g;
    if (f.lds_form) {
        int per_cu = (int)(SDNR_LDS_PER_CU / (f.lds ? f.lds : 1));
        per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);     // 2048 threads per CU
        g = (int64_t)ctx->num_cus * per_cu;
    } else {
        g = (int64_t)ctx->num_cus * 2;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / f.stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
    }
    if (g > nrows) g = nrows;
    f.grid = g;
    return f;
}

}  // namespace

#endif  // SDNR_ECMP_FAIR_ROWS_H
