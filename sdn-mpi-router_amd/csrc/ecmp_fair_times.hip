// ecmp_fair_times.hip -- max-min fair completion times over ECMP: when every
// flow of an exchange ends if each is split over EVERY least-cost route, where
// fair_times.hip puts every flow on one path.  The flows, fractions and the
// filling are ecmp_fair_rates.hip's; a flow that has sent its bytes leaves and
// the others are refilled.  Epoch j = 0, 1, ... over the flows in flight
// (rem_b = bytes, t = 0, carried = 0 at the start):
//   1. fill: the progressive filling of ecmp_fair_rates.hip, unchanged (steps
//      1-5, the tie tolerance kFairTie and the closing step 2), gives rate[i],
//      used[e] and the epoch's round count (rate0 = the rates of epoch 0);
//   2. advance: q[i] = rem_b[i] / rate[i], dt = min q, bound = dt + dt *
//      kFairTie (ef_tie_bound: two roundings), t_j = t_{j-1} + dt, carried[e] +=
//      used[e] * dt (the multiply and the add rounded one by one); a flow
//      finishes iff q[i] <= bound or rem_b[i] - rate[i] * dt <= 0.0 (multiply
//      and subtract rounded one by one): time = t_j, epoch = j; otherwise
//      rem_b[i] becomes that difference;
//   3. end when nothing is in flight; every epoch removes a flow.
// The definition is sdnroute.h's (sdnr_ecmp_fair_times); engine.
// ecmp_fair_times_host restates it.  The advance shares the filling's tolerance
// because a[e] is a float sum whose adds arrive in any order: the levels, and
// with them the q of flows that end together as fractions, differ in their
// last bits between two runs.  An exact q == dt would let such flows leave in
// one epoch here and in two there, each spurious epoch a full refill with its
// DAG sweeps; with the tolerance membership flips only at q ~ dt * (1 + 2^-30).
//
// The clock of fair_times.hip (fair_epochs.h's FairClock: phase, epoch, round)
// lives in device memory and tells every queued launch what to do; only the
// last workgroup of an entry pass advances it.  No grid-wide barrier and no
// waiting between workgroups.  A step is two launches:
//   ecmp_fair_times_rows_kernel, ecmp_fair_rows.h's row pass, persistent over
//     rows:
//     phase fill, round k: the verdict of round k - 1 and the counts of round
//       k; round 0 of epoch 0 classifies the flows, round 0 of a later epoch
//       applies the dt of the epoch before (finish or subtract) in the same
//       pass that counts;
//     phase advance: the minimum of q over the row's flows, atomicMin on the
//       bits into the clock's dt (inside the body's row loop).
//     Round 0 of epoch max_epochs only applies the last advance and marks the
//     flows still in flight: the call is capped after it, so it counts nothing.
//     A row with nothing in flight returns before it reads its pcost row.
//   ecmp_fair_times_entries_kernel, over the E + nextra entries:
//     phase fill: ecmp_fair_rows.h's link step and the clamp of the level; the
//       last workgroup goes on to round k + 1, or -- level[k] = +inf -- to the
//       advance (k = 0: nothing is in flight, the call is done); in round 0 of
//       epoch max_epochs it stops the call as capped;
//     phase advance: carried += used * dt, rem = cap, used = 0, a = a_prev = 0,
//       share = level = +inf; the last workgroup stores t_j and the epoch's
//       rounds and goes on to round 0 of epoch j + 1.
// Epoch j with K_j rounds takes K_j + 2 steps (rounds 0 .. K_j and the advance)
// and the round 0 that finds nothing in flight, or the cap, one more.  The
// host queues kFairBatch steps, reads the clock's four words back, and stops
// when the phase says done or capped; steps queued behind that return at once.
// Depth and sigma of a row are redone in every visit, as in ecmp_fair_rates.hip.
#include "ecmp_fair_rows.h"

namespace {

__global__ __launch_bounds__(kEcmpFairLinkThreads) void ecmp_fair_times_init_kernel(
    EcmpFairState s, FairClock *__restrict__ clock, FairTimes ft, const double *__restrict__ cap,
    double *__restrict__ carried, double *__restrict__ rate, int32_t *__restrict__ round,
    int n_ent, int nlevel, int nrows, int64_t pair_lo, int64_t pair_hi, int *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * kEcmpFairLinkThreads + threadIdx.x;
    const double inf = __longlong_as_double((long long)kInfBits);
    if (i < n_ent) {
        s.rem[i] = fair_capacity(cap[i], err, kErrEcmpFairTimes);
        s.used[i] = 0.0;
        s.share[i] = inf;
        s.a[i] = 0.0;
        s.a_prev[i] = 0.0;
        carried[i] = 0.0;
    }
    if (i < nlevel) s.level[i] = kInfBits;
    if (i < nrows) {
        s.alive_row[i] = 0;
        ft.inflight_row[i] = 0;
    }
    if (i < pair_hi - pair_lo) {
        // every flow is absent until a row says otherwise
        const int64_t p = pair_lo + i;
        const double nb = ft.bytes[p];
        if (!(nb >= 0.0) || nb == inf) atomicOr(err, kErrEcmpFairTimes);   // negative or not finite
        ft.time[p] = inf;
        ft.epoch[p] = -1;
        ft.rate0[p] = 0.0;
        ft.remaining[p] = nb;
        rate[p] = 0.0;
        round[p] = -1;
    }
    if (i == 0) {
        *s.status = 0;
        *s.ticket = 0;
        clock->phase = kPhaseFill;
        clock->epoch = 0;
        clock->round = 0;
        clock->nepochs = 0;
        clock->t = 0.0;
        clock->dt[0] = kInfBits;
        clock->dt[1] = kInfBits;
    }
}

template <bool LDS>
__global__ __launch_bounds__(kEcmpFairThreads) void ecmp_fair_times_rows_kernel(
    int V, int E, int nextra, int nrows, int hop, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const uint32_t *__restrict__ cost,
    const uint32_t *__restrict__ pcost, const int64_t *__restrict__ pair_off, int64_t pair_lo,
    int64_t pair_hi, const int32_t *__restrict__ srcs, const uint64_t *__restrict__ mult,
    const int32_t *__restrict__ extra, EcmpFairState s, FairClock *__restrict__ clock,
    FairTimes ft, double *__restrict__ rate, int32_t *__restrict__ round,
    unsigned char *__restrict__ scratch, size_t scratch_stride, int *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ecmp_fair_lds[];
    __shared__ unsigned long long s_alive;
    const int phase = clock->phase;
    if (phase >= kPhaseDone) return;                       // the call ended before this step
    const int j = clock->epoch;
    ft.j = j;
    ft.dt = j > 0 ? __longlong_as_double((long long)clock->dt[(j - 1) & 1]) : 0.0;
    ft.t = clock->t;
    // (the advance phase runs inside the body's row loop: with a row loop of
    // its own here the kernel kept a private segment that nothing touched)
    const bool advance = phase == kPhaseAdvance;
    ecmp_fair_rows_body<LDS, true>(V, E, nextra, nrows, hop, advance ? 0 : clock->round, row_ptr,
                                   col, cost, pcost, pair_off, pair_lo, pair_hi, srcs, mult, extra,
                                   s, rate, (int32_t *)nullptr, round, scratch, scratch_stride,
                                   err, kErrEcmpFairTimes, ft,
                                   advance ? &clock->dt[j & 1] : nullptr, ecmp_fair_lds, &s_alive);
}

__global__ __launch_bounds__(kEcmpFairLinkThreads) void ecmp_fair_times_entries_kernel(
    EcmpFairState s, FairClock *__restrict__ clock, const double *__restrict__ cap,
    double *__restrict__ carried, double *__restrict__ epoch_time,
    int32_t *__restrict__ epoch_rounds, int n_ent, int nlevel, int max_epochs,
    int *__restrict__ err)
{
    const int phase = clock->phase;
    if (phase >= kPhaseDone) return;                       // the call ended before this step
    const int j = clock->epoch, k = clock->round;
    const unsigned long long dtb = clock->dt[j & 1];
    if (phase == kPhaseFill) {
        ecmp_fair_links_step(s, n_ent, k);
    } else {
        const int i = (int)(blockIdx.x * (unsigned)kEcmpFairLinkThreads + threadIdx.x);
        if (i < n_ent) {
            if (dtb != kInfBits)
                carried[i] = fair_carry(carried[i], s.used[i], __longlong_as_double((long long)dtb));
            s.rem[i] = fair_capacity(cap[i], err, kErrEcmpFairTimes);
            s.used[i] = 0.0;
            s.share[i] = __longlong_as_double((long long)kInfBits);
            s.a[i] = 0.0;
            s.a_prev[i] = 0.0;
        }
        if (i < nlevel) s.level[i] = kInfBits;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(s.ticket, 1u) == gridDim.x - 1) {    // the last workgroup of the pass
            __threadfence();
            *s.ticket = 0;
            if (phase == kPhaseFill) {
                const bool end = ecmp_fair_close_level(s, k);
                if (k == 0 && j == max_epochs) {           // (the row pass made no counts)
                    clock->nepochs = max_epochs;
                    clock->phase = kPhaseCapped;
                } else if (end && k == 0) {                // nothing in flight
                    clock->nepochs = j;
                    clock->phase = kPhaseDone;
                } else if (end) {
                    clock->phase = kPhaseAdvance;          // (round stays K_j, the epoch's rounds)
                } else if (k + 1 >= nlevel) {              // (every round freezes a flow and
                    clock->nepochs = j;                    // empties a link: not reached)
                    clock->phase = kPhaseDone;
                } else {
                    clock->round = k + 1;
                }
            } else if (dtb == kInfBits) {                  // no flow was frozen: nothing can end
                clock->nepochs = j;
                clock->phase = kPhaseDone;
            } else {
                const double tj = clock->t + __longlong_as_double((long long)dtb);
                clock->t = tj;
                epoch_time[j] = tj;
                epoch_rounds[j] = k;
                clock->dt[(j + 1) & 1] = kInfBits;
                clock->epoch = j + 1;
                clock->round = 0;
                clock->phase = kPhaseFill;
            }
        }
    }
}

}  // namespace

int sdnr_launch_ecmp_fair_times(sdnr_ctx *ctx, const uint32_t *d_pcost, int32_t nrows,
                                const int64_t *d_pair_off, int64_t pair_lo, int64_t pair_hi,
                                const int32_t *d_srcs, const uint64_t *d_mult,
                                const double *d_bytes, const int32_t *d_extra, const double *d_cap,
                                int32_t nextra, double *d_time, int32_t *d_epoch, double *d_rate0,
                                double *d_remaining, double *d_epoch_time,
                                int32_t *d_epoch_rounds, int32_t max_epochs, double *d_carried,
                                int32_t *nepochs, bool hop)
{
    const int V = ctx->V;
    const int n_ent = ctx->E + nextra;
    const size_t npairs = (size_t)(pair_hi - pair_lo);
    const uint32_t *cost = ctx->has_cost ? ctx->cost : nullptr;   // none: every link costs 1
    const EcmpFairShape shape = ecmp_fair_shape(ctx, nrows);
    const size_t lds = shape.lds, stride = shape.stride;
    const int64_t g = shape.grid;

    // behind the slices: a, a_prev, rem, share, used, level, alive_row,
    // inflight_row, status, ticket, the clock, then the flows' rate and round
    const size_t max_rounds = npairs < (size_t)n_ent ? npairs : (size_t)n_ent;
    const size_t slices = (stride * (size_t)g + 255) & ~(size_t)255;
    const size_t nlevel = max_rounds + 1;
    const size_t words = 5 * (size_t)n_ent + nlevel + 2 * (size_t)nrows + 2 +
                         sizeof(FairClock) / 8 + npairs + (npairs + 1) / 2;
    const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, slices + 8 * words);
    if (rc) return rc;
    unsigned char *base = static_cast<unsigned char *>(ctx->scratch);
    EcmpFairState s;
    s.a = reinterpret_cast<double *>(base + slices);
    s.a_prev = s.a + n_ent;
    s.rem = s.a_prev + n_ent;
    s.share = s.rem + n_ent;
    s.used = s.share + n_ent;
    s.level = reinterpret_cast<unsigned long long *>(s.used + n_ent);
    s.alive_row = reinterpret_cast<long long *>(s.level + nlevel);
    FairTimes ft{};
    ft.inflight_row = s.alive_row + nrows;
    s.status = reinterpret_cast<unsigned long long *>(ft.inflight_row + nrows);
    s.ticket = reinterpret_cast<unsigned int *>(s.status + 1);
    FairClock *clock = reinterpret_cast<FairClock *>(s.status + 2);
    // (indexed by the flow's place in the caller's lists, which start at pair_lo)
    double *rate = reinterpret_cast<double *>(clock + 1) - pair_lo;
    int32_t *round = reinterpret_cast<int32_t *>(rate + pair_lo + npairs) - pair_lo;
    ft.bytes = d_bytes;
    ft.remaining = d_remaining;
    ft.time = d_time;
    ft.epoch = d_epoch;
    ft.rate0 = d_rate0;
    ft.max_epochs = max_epochs;

    hipStream_t st = ctx->stream;
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, st));
    size_t init_n = (size_t)n_ent > nlevel ? (size_t)n_ent : nlevel;
    if (init_n < npairs) init_n = npairs;
    if (init_n < (size_t)nrows) init_n = (size_t)nrows;
    const size_t ent_n = (size_t)n_ent > nlevel ? (size_t)n_ent : nlevel;
    const unsigned ent_blocks =
        (unsigned)((ent_n + kEcmpFairLinkThreads - 1) / kEcmpFairLinkThreads);
    hipLaunchKernelGGL(ecmp_fair_times_init_kernel,
                       dim3((unsigned)((init_n + kEcmpFairLinkThreads - 1) / kEcmpFairLinkThreads)),
                       dim3(kEcmpFairLinkThreads), 0, st, s, clock, ft, d_cap, d_carried, rate,
                       round, n_ent, (int)nlevel, nrows, pair_lo, pair_hi, ctx->d_err);
    SDNR_HIP(hipGetLastError());
    int launches = 1;
    auto fn_lds = ecmp_fair_times_rows_kernel<true>;
    if (shape.lds_form) sdnr_allow_lds(reinterpret_cast<const void *>(fn_lds), lds);
    ctx->last_kernel = shape.lds_form ? "ecmp_fair_times_rows_kernel<lds>"
                                      : "ecmp_fair_times_rows_kernel<global>";
    ctx->last_grid = g;

    // every epoch removes a flow and every round freezes one: more steps than
    // this cannot be needed
    const long long most = ((long long)max_epochs + 1) * ((long long)max_rounds + 2) + 1;
    long long steps = 0;
    int word[4] = {0, 0, 0, 0};
    while (word[0] < kPhaseDone) {
        if (steps > most)
            return sdnr_fail(SDNR_ERR_HIP,
                             "sdnr_ecmp_fair_times: the clock did not stop in %lld steps", steps);
        for (int b = 0; b < kFairBatch; ++b) {
            if (shape.lds_form)
                hipLaunchKernelGGL(fn_lds, dim3((unsigned)g), dim3(kEcmpFairThreads), lds, st, V,
                                   ctx->E, nextra, nrows, hop ? 1 : 0, ctx->row_ptr, ctx->col, cost,
                                   d_pcost, d_pair_off, pair_lo, pair_hi, d_srcs, d_mult, d_extra,
                                   s, clock, ft, rate, round, (unsigned char *)nullptr, (size_t)0,
                                   ctx->d_err);
            else
                hipLaunchKernelGGL(ecmp_fair_times_rows_kernel<false>, dim3((unsigned)g),
                                   dim3(kEcmpFairThreads), 0, st, V, ctx->E, nextra, nrows,
                                   hop ? 1 : 0, ctx->row_ptr, ctx->col, cost, d_pcost, d_pair_off,
                                   pair_lo, pair_hi, d_srcs, d_mult, d_extra, s, clock, ft, rate,
                                   round, base, stride, ctx->d_err);
            hipLaunchKernelGGL(ecmp_fair_times_entries_kernel, dim3(ent_blocks),
                               dim3(kEcmpFairLinkThreads), 0, st, s, clock, d_cap, d_carried,
                               d_epoch_time, d_epoch_rounds, n_ent, (int)nlevel, max_epochs,
                               ctx->d_err);
        }
        steps += kFairBatch;
        launches += 2 * kFairBatch;
        SDNR_HIP(hipGetLastError());
        const int rf = sdnr_fetch_ints(ctx, reinterpret_cast<const int *>(clock), 4, word);
        if (rf) return rf;
    }
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, st));
    ctx->last_launches = launches;
    *nepochs = word[3];
    return SDNR_OK;
}
