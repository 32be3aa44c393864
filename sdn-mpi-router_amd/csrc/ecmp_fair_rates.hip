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
//
// The row pass, the link step and the launch shape live in ecmp_fair_rows.h,
// which ecmp_fair_times.hip (a filling per departure epoch) runs too.
#include "ecmp_fair_rows.h"

namespace {

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

// the body is ecmp_fair_rows.h's, which sdnr_ecmp_fair_times runs too
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
    extern __shared__ __attribute__((aligned(16))) unsigned char ecmp_fair_lds[];
    __shared__ unsigned long long s_alive;
    if (k > 0 && *s.status) return;                        // the rounds ended before this one
    const FairTimes none{};
    ecmp_fair_rows_body<LDS, false>(V, E, nextra, nrows, hop, k, row_ptr, col, cost, pcost,
                                    pair_off, pair_lo, pair_hi, srcs, mult, extra, s, rate, bott,
                                    round, scratch, scratch_stride, err, kErrEcmpFairRates, none,
                                    nullptr, ecmp_fair_lds, &s_alive);
}

__global__ __launch_bounds__(kEcmpFairLinkThreads) void ecmp_fair_links_kernel(EcmpFairState s,
                                                                             int n_ent, int k)
{
    if (k > 0 && *s.status) return;                        // the rounds ended before this one
    ecmp_fair_links_step(s, n_ent, k);
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(s.ticket, 1u) == gridDim.x - 1) {    // the last workgroup of the pass
            __threadfence();
            *s.ticket = 0;
            if (ecmp_fair_close_level(s, k)) *s.status = (unsigned long long)k + 1;
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
    const EcmpFairShape shape = ecmp_fair_shape(ctx, nrows);
    const bool lds_form = shape.lds_form;
    const size_t lds = shape.lds, stride = shape.stride;
    const int64_t g = shape.grid;

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
