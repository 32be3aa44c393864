// ecmp_fair_rates.hip -- max-min fair flow rates of flows split over EVERY
// least-cost route (ECMP), where fair_rates.hip puts every flow on one path.
//
// A flow is a pair of sdnr_cost_ecmp_link_loads (least-cost row r toward one
// destination, source vertex s) with a multiplicity and up to two extra
// constraints (host ports).  Link e = (x -> n) is tight in the row when
// pcost[n] != INF and pcost[n] + cost[e] == pcost[x]; the flow crosses every
// tight link reachable from s over tight links, and puts on it the fraction
// phi(e) that cost_ecmp_loads.hip would put there for unit weight (route split:
// sigma[n] / sigma[x] down the DAG; hop split: 1 / next hops).  Without
// uploaded costs every link costs 1: hop-count ECMP.  With rem = cap, used = 0,
// a_prev = 0, r_{-1} = 0, round k = 0, 1, ...:
//   1. a[e]  = sum over the alive flows of mult * phi(e) (f64: the ECMP push of
//      the alive multiplicities; an extra: the alive multiplicity itself);
//   2. k > 0: m = max(a_prev[e] - a[e], 0), p = r_{k-1} * m, used[e] += p,
//      rem[e] = max(rem[e] - p, 0)            (each operation rounded alone);
//   3. share[e] = rem[e] / a[e] (a[e] > 0, else +inf),
//      r_k = max(min share, r_{k-1}); r_k = +inf: stop;
//   4. e is saturated iff share[e] <= r_k + r_k * kFairTie (two roundings);
//      every alive flow that crosses a saturated link or has a saturated extra
//      gets rate r_k, round k and bott = the smallest saturated link index it
//      crosses, else extra 0, else extra 1, and is dead; a_prev = a.
// a[e] is a float sum, so two links whose shares are equal as fractions differ
// in their last bits -- under ECMP on a symmetric fabric every link of a tier.
// The exact tie of fair_rates.hip would freeze each in a round of its own; the
// tolerance kFairTie = 2^-30 (the project's 1e-9) freezes them together, and
// the clamp of step 3 keeps the levels from falling.
//
// No grid-wide barrier and no waiting between workgroups: a round is two plain
// launches on the context's stream, as in fair_rates.hip.
//   ecmp_fair_rows_kernel (round k), one workgroup per row, persistent over the
//     rows.  A row visit orders the vertices by their longest next-hop chain
//     and counts the routes (the pull sweeps of cost_ecmp_loads.hip, redone
//     every round: nothing per row is kept between rounds but its alive count),
//     then
//     (a) the verdict of round k - 1, by ascending depth, gathers only:
//         B[x] = min over the tight links (x -> n) of (saturated(e) ? e : none,
//         B[n]); the row's alive flows read B[src], then their extras, and
//         store rate, round and bott;
//     (b) the counts of round k: flow[] is seeded with the alive multiplicities
//         and pushed by descending depth, f64 adds into flow[n] (LDS or
//         scratch) and a[e] (global), one add per alive flow's extra.
//     Round 0 classifies the flows instead of (a).  B (i32) aliases flow, which
//     (b) seeds only after (a) is done.  A row whose alive counter is 0 returns
//     before reading anything.  Row state: LDS (f64 sigma + f64 flow + u32
//     pcost + u16 depth, kEcmpFairBytesPerV = 22 bytes per vertex) up to
//     kEcmpFairLdsMaxV vertices, else a per-workgroup slice of the context
//     scratch (sigma, flow and u32 depth, 20 bytes per vertex).
//   ecmp_fair_links_kernel (round k), over the E + nextra entries: step 2,
//     share, a_prev = a, a = 0, a wave-reduced minimum into level[k]; the last
//     workgroup to finish clamps level[k] to level[k - 1] and stores k + 1 into
//     the status word if it is +inf.  A kernel launched after that returns.
// The host queues kFairBatch rounds, reads the 8-byte status word back, and
// goes on until it is set (or max_rounds rounds were run).
//
// The adds into a[e] arrive in any order: results equal the host restatement
// (engine.ecmp_fair_rates_host) within rounding, and bit for bit where every
// partial sum is exact.
#include "common.h"

namespace {

constexpr int kEcmpFairThreads = 1024;   // chains of dependent LDS / L2 reads, as cost_ecmp_loads.hip
constexpr int kEcmpFairLinkThreads = 256;
constexpr int kFairBatch = 16;           // rounds queued per status read-back
constexpr int kFairAlive = -2;           // round[] of a flow not frozen yet
constexpr double kFairTie = 0x1p-30;     // shares within r_k * kFairTie of r_k tie with it
constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;
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
// and the add rounded one by one as the host's numpy does
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

__global__ __launch_bounds__(kEcmpFairLinkThreads) void ecmp_fair_init_kernel(
    EcmpFairState s, const double *__restrict__ cap, int n_ent, int nlevel, int *__restrict__ err)
{
    const int i = (int)(blockIdx.x * (unsigned)kEcmpFairLinkThreads + threadIdx.x);
    if (i < n_ent) {
        double c = cap[i];
        if (!(c > 0.0) || __double_as_longlong(c) == (long long)kInfBits) {
            atomicOr(err, kErrEcmpFairRates);              // not positive and finite
            c = __longlong_as_double((long long)kInfBits); // (never saturates: results invalid)
        }
        s.rem[i] = c;
        s.used[i] = 0.0;
        s.share[i] = __longlong_as_double((long long)kInfBits);
        s.a[i] = 0.0;
        s.a_prev[i] = 0.0;
    }
    if (i < nlevel) s.level[i] = kInfBits;
    if (i == 0) {
        *s.status = 0;
        *s.ticket = 0;
    }
}

// hop: sigma[x] holds the number of next hops instead of the route count;
// cost NULL: every link costs 1
template <bool LDS>
__global__ __launch_bounds__(kEcmpFairThreads) void ecmp_fair_rows_kernel(
    int V, int E, int nextra, int nrows, int hop, int k, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const uint32_t *__restrict__ cost,
    const uint32_t *__restrict__ pcost, const int64_t *__restrict__ pair_off, int64_t pair_lo,
    int64_t pair_hi, const int32_t *__restrict__ srcs, const uint64_t *__restrict__ mult,
    const int32_t *__restrict__ extra, EcmpFairState s, double *__restrict__ rate,
    int32_t *__restrict__ bott, int32_t *__restrict__ round, unsigned char *__restrict__ scratch,
    size_t scratch_stride, int *__restrict__ err)
{
    typedef EfDepth<LDS> Dp;
    typedef typename Dp::T depth_t;
    // dynamic LDS, LDS form: sigma f64 [V] | flow f64 [V] | pcost u32 [V] | depth u16 [V]
    extern __shared__ __attribute__((aligned(16))) unsigned char ecmp_fair_lds[];
    __shared__ unsigned long long s_alive;
    if (k > 0 && *s.status) return;                        // the rounds ended before this one
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
            if (tid == 0) atomicOr(err, kErrEcmpFairRates);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no flow)
        if (k > 0 && s.alive_row[r] == 0) continue;        // (uniform: none of them alive)
        const uint32_t *prow = pcost + (size_t)r * (size_t)V;
        const uint32_t *pc = LDS ? pc_lds : prow;

        // 1. the destination (pcost 0) and the unreachable are final at depth 0
        for (int x = tid; x < V; x += kEcmpFairThreads) {
            const uint32_t px = prow[x];
            if (LDS) pc_lds[x] = px;
            ef_st_f64<LDS>(&sigma[x], (px == 0 && !hop) ? 1.0 : 0.0);
            Dp::st(&depth[x], (px == 0 || px == kEfInf) ? 0 : Dp::kPending);
        }
        if (tid == 0) s_alive = 0;
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
        // stay 0.0 / -1 / -1 and it contributes nothing)
        if (k == 0 && __syncthreads_or(bad ? 1 : 0)) {
            if (tid == 0) {
                atomicOr(err, kErrEcmpFairRates);
                s.alive_row[r] = 0;
            }
            continue;
        }

        unsigned long long mine = 0;                       // this thread's flows still alive
        if (k == 0) {
            // classify the row's flows (rate 0.0, bott -1, round -1 are preset)
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
                        atomicOr(err, kErrEcmpFairRates);  // (that constraint is ignored)
                }
                if (px == 0 && ef_extra(extra, i, 0, E, nextra) < 0 &&
                    ef_extra(extra, i, 1, E, nextra) < 0) {
                    rate[i] = inf;                         // s == d and no extra
                    continue;
                }
                round[i] = kFairAlive;
                ++mine;
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
                    bott[i] = b;
                    round[i] = k - 1;
                } else {
                    ++mine;
                }
            }
        }
        if (mine) atomicAdd(&s_alive, mine);
        __syncthreads();                                   // (B is read; flow may be seeded)
        const unsigned long long alive = s_alive;
        if (tid == 0) s.alive_row[r] = (long long)alive;
        if (alive == 0) {
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

__global__ __launch_bounds__(kEcmpFairLinkThreads) void ecmp_fair_links_kernel(EcmpFairState s,
                                                                             int n_ent, int k)
{
    // the subtract, the multiply, the add and the subtract of step 2 round one
    // by one, as the host's numpy does: no fused multiply-add
#pragma clang fp contract(off)
    if (k > 0 && *s.status) return;                        // the rounds ended before this one
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
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(s.ticket, 1u) == gridDim.x - 1) {    // the last workgroup of the pass
            __threadfence();
            *s.ticket = 0;
            const unsigned long long lv =
                __hip_atomic_load(&s.level[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lv == kInfBits)
                *s.status = (unsigned long long)k + 1;
            else if (k > 0 && lv < s.level[k - 1])         // r_k = max(min share, r_{k-1})
                s.level[k] = s.level[k - 1];
        }
    }
}

}  // namespace

int sdnr_launch_ecmp_fair_rates(sdnr_ctx *ctx, const uint32_t *d_pcost, int32_t nrows,
                                const int64_t *d_pair_off, int64_t pair_lo, int64_t pair_hi,
                                const int32_t *d_srcs, const uint64_t *d_mult,
                                const int32_t *d_extra, const double *d_cap, int32_t nextra,
                                double *d_rate, int32_t *d_bott, int32_t *d_round, double *d_level,
                                int32_t max_rounds, double *d_used, int32_t *nrounds, bool hop)
{
    const int V = ctx->V;
    const int n_ent = ctx->E + nextra;
    const size_t npairs = (size_t)(pair_hi - pair_lo);
    const uint32_t *cost = ctx->has_cost ? ctx->cost : nullptr;   // none: every link costs 1

    // the row kernel's shape, and its per-workgroup scratch slices
    const bool lds_form = V <= kEcmpFairLdsMaxV;
    const size_t lds = lds_form ? (((size_t)V * kEcmpFairBytesPerV + 15) & ~(size_t)15) : 0;
    const size_t stride = lds_form ? 0 : ((((size_t)V * 20) + 255) & ~(size_t)255);
    int64_t g;
    if (lds_form) {
        int per_cu = (int)(SDNR_LDS_PER_CU / (lds ? lds : 1));
        per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);     // 2048 threads per CU
        g = (int64_t)ctx->num_cus * per_cu;
    } else {
        g = (int64_t)ctx->num_cus * 2;
        const int64_t fit = (int64_t)(kLoadsScratchBytes / stride);
        if (g > fit) g = fit < 1 ? 1 : fit;
    }
    if (g > nrows) g = nrows;

    // the state behind the slices: a, a_prev, rem, share, level, alive_row, status, ticket
    const size_t slices = (stride * (size_t)g + 255) & ~(size_t)255;
    const size_t nlevel = (size_t)max_rounds + 1;
    const size_t state = 8 * (4 * (size_t)n_ent + nlevel + (size_t)nrows + 2);
    const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, slices + state);
    if (rc) return rc;
    unsigned char *base = static_cast<unsigned char *>(ctx->scratch);
    EcmpFairState s;
    s.a = reinterpret_cast<double *>(base + slices);
    s.a_prev = s.a + n_ent;
    s.rem = s.a_prev + n_ent;
    s.share = s.rem + n_ent;
    s.level = reinterpret_cast<unsigned long long *>(s.share + n_ent);
    s.alive_row = reinterpret_cast<long long *>(s.level + nlevel);
    s.status = reinterpret_cast<unsigned long long *>(s.alive_row + nrows);
    s.ticket = reinterpret_cast<unsigned int *>(s.status + 1);
    s.used = d_used;

    hipStream_t st = ctx->stream;
    // every flow reads 0.0 / -1 / -1 until a row says otherwise
    SDNR_HIP(hipMemsetAsync(d_rate + pair_lo, 0, npairs * sizeof(double), st));
    SDNR_HIP(hipMemsetAsync(d_bott + pair_lo, 0xFF, npairs * sizeof(int32_t), st));
    SDNR_HIP(hipMemsetAsync(d_round + pair_lo, 0xFF, npairs * sizeof(int32_t), st));
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, st));
    const size_t init_n = (size_t)n_ent > nlevel ? (size_t)n_ent : nlevel;
    unsigned link_blocks =
        (unsigned)((n_ent + kEcmpFairLinkThreads - 1) / kEcmpFairLinkThreads);
    if (link_blocks == 0) link_blocks = 1;                 // (no link, no extra: level[0] = +inf)
    hipLaunchKernelGGL(ecmp_fair_init_kernel,
                       dim3((unsigned)((init_n + kEcmpFairLinkThreads - 1) / kEcmpFairLinkThreads)),
                       dim3(kEcmpFairLinkThreads), 0, st, s, d_cap, n_ent, (int)nlevel,
                       ctx->d_err);
    SDNR_HIP(hipGetLastError());
    int launches = 1;
    auto fn_lds = ecmp_fair_rows_kernel<true>;
    if (lds_form) sdnr_allow_lds(reinterpret_cast<const void *>(fn_lds), lds);
    ctx->last_kernel = lds_form ? "ecmp_fair_rows_kernel<lds>" : "ecmp_fair_rows_kernel<global>";
    ctx->last_grid = g;

    int k = 0, done = -1;
    while (done < 0) {
        // rounds 0 .. max_rounds: the last one only applies the verdict of
        // round max_rounds - 1 and makes used final
        const int end = k + kFairBatch <= max_rounds + 1 ? k + kFairBatch : max_rounds + 1;
        for (; k < end; ++k) {
            if (lds_form)
                hipLaunchKernelGGL(fn_lds, dim3((unsigned)g), dim3(kEcmpFairThreads), lds, st, V,
                                   ctx->E, nextra, nrows, hop ? 1 : 0, k, ctx->row_ptr, ctx->col,
                                   cost, d_pcost, d_pair_off, pair_lo, pair_hi, d_srcs, d_mult,
                                   d_extra, s, d_rate, d_bott, d_round, (unsigned char *)nullptr,
                                   (size_t)0, ctx->d_err);
            else
                hipLaunchKernelGGL(ecmp_fair_rows_kernel<false>, dim3((unsigned)g),
                                   dim3(kEcmpFairThreads), 0, st, V, ctx->E, nextra, nrows,
                                   hop ? 1 : 0, k, ctx->row_ptr, ctx->col, cost, d_pcost,
                                   d_pair_off, pair_lo, pair_hi, d_srcs, d_mult, d_extra, s, d_rate,
                                   d_bott, d_round, base, stride, ctx->d_err);
            hipLaunchKernelGGL(ecmp_fair_links_kernel, dim3(link_blocks),
                               dim3(kEcmpFairLinkThreads), 0, st, s, n_ent, k);
            launches += 2;
        }
        SDNR_HIP(hipGetLastError());
        int word[2];
        const int rf = sdnr_fetch_ints(ctx, reinterpret_cast<const int *>(s.status), 2, word);
        if (rf) return rf;
        const unsigned long long status =
            ((unsigned long long)(uint32_t)word[1] << 32) | (uint32_t)word[0];
        if (status) done = (int)(status - 1);
        else if (k > max_rounds) done = max_rounds;        // flows left alive keep round -2
    }
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, st));
    if (max_rounds > 0)
        SDNR_HIP(hipMemcpyAsync(d_level, s.level, (size_t)max_rounds * sizeof(double),
                                hipMemcpyDeviceToDevice, st));
    ctx->last_launches = launches;
    *nrounds = done < max_rounds ? done : max_rounds;
    return SDNR_OK;
}
