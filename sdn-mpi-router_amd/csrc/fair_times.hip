// fair_times.hip -- max-min fair completion times: when every flow of an
// exchange ends in the fluid model behind fair_rates.hip.  The flows share
// max-min fairly; a flow that has sent its bytes leaves and the others are
// refilled.  Epoch j = 0, 1, ... over the flows in flight (rem_b = bytes,
// t = 0, carried = 0 at the start):
//   1. fill: the progressive filling of fair_rates.hip, unchanged, gives
//      rate[i], used[e] and the epoch's round count (rate0 = the rates of
//      epoch 0);
//   2. advance: q[i] = rem_b[i] / rate[i], dt = min q, t_j = t_{j-1} + dt,
//      carried[e] += used[e] * dt (the multiply and the add rounded one by
//      one); a flow finishes iff q[i] == dt or rem_b[i] - rate[i] * dt <= 0.0
//      (multiply and subtract rounded one by one): time = t_j, epoch = j;
//      otherwise rem_b[i] becomes that difference;
//   3. end when nothing is in flight; every epoch removes a flow.
// The definition is sdnroute.h's (sdnr_fair_times); engine.fair_times_host
// restates it and agrees bit for bit.
//
// The host knows neither the round nor the epoch.  A clock in device memory
// (phase, epoch, round) tells every queued launch what to do, and only the last
// workgroup of an entry pass advances it (the ticket of fair_links_kernel), so
// the next launch on the stream sees it.  No grid-wide barrier and no waiting
// between workgroups.  A step is two launches:
//   fair_times_rows_kernel, fair_rows.h's row pass, persistent over rows:
//     phase fill, round k: the verdict of round k - 1 and the counts of round
//       k; round 0 of epoch 0 classifies the flows, round 0 of a later epoch
//       applies the dt of the epoch before (finish or subtract) in the same
//       pass that counts;
//     phase advance: the minimum of q over the row's flows, atomicMin on the
//       bits into the clock's dt.
//   fair_times_entries_kernel, over the E + nextra entries:
//     phase fill: fair_rows.h's entry step; the last workgroup goes on to round
//       k + 1, or -- level[k] = +inf -- to the advance (k = 0: nothing is in
//       flight, the call is done); in round 0 of epoch max_epochs it stops the
//       call as capped;
//     phase advance: carried += used * dt, rem = cap, used = 0, n_prev = 0,
//       share = level = +inf; the last workgroup stores t_j and the epoch's
//       rounds and goes on to round 0 of epoch j + 1.
// Epoch j with K_j rounds takes K_j + 2 steps (rounds 0 .. K_j and the advance)
// and the round 0 that finds nothing in flight, or the cap, one more.  The
// host queues kFairBatch steps, reads the clock's four words back, and stops
// when the phase says done or capped; steps queued behind that return at once.
// e_v is looked up again in every row visit, as in fair_rates.hip.
#include "fair_rows.h"

namespace {

__global__ __launch_bounds__(kFairLinkThreads) void fair_times_init_kernel(
    FairState s, FairClock *__restrict__ clock, FairTimes ft, const double *__restrict__ cap,
    double *__restrict__ carried, double *__restrict__ rate, int32_t *__restrict__ round,
    int n_ent, int nlevel, int nrows, int64_t pair_lo, int64_t pair_hi, int *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * kFairLinkThreads + threadIdx.x;
    const double inf = __longlong_as_double((long long)kInfBits);
    if (i < n_ent) {
        s.rem[i] = fair_capacity(cap[i], err, kErrFairTimes);
        s.used[i] = 0.0;
        s.share[i] = inf;
        s.n[i] = 0;
        s.n_prev[i] = 0;
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
        if (!(nb >= 0.0) || nb == inf) atomicOr(err, kErrFairTimes);   // negative or not finite
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

template <typename JT, bool LDS>
__global__ __launch_bounds__(kFairThreads) void fair_times_rows_kernel(
    FairRows t, int V, int E, int nextra, int nrows, int max_steps,
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int64_t *__restrict__ pair_off, int64_t pair_lo, int64_t pair_hi,
    const int32_t *__restrict__ verts, const uint64_t *__restrict__ mult,
    const int32_t *__restrict__ extra, FairState s, FairClock *__restrict__ clock, FairTimes ft,
    double *__restrict__ rate, int32_t *__restrict__ round, unsigned char *__restrict__ scratch,
    size_t scratch_stride, int *__restrict__ err)
{
    extern __shared__ unsigned long long fair_lds[];
    __shared__ unsigned long long s_alive;
    const int phase = clock->phase;
    if (phase >= kPhaseDone) return;                       // the call ended before this step
    const int j = clock->epoch;
    if (phase == kPhaseAdvance) {
        // dt = min q over the flows in flight (all frozen by now)
        for (int r = (int)blockIdx.x; r < nrows; r += (int)gridDim.x) {
            if (ft.inflight_row[r] == 0) continue;         // (also: a row with bad offsets)
            const int64_t lo = pair_off[r], hi = pair_off[r + 1];
            if (lo < pair_lo || hi > pair_hi || hi < lo) continue;
            unsigned long long bits = kInfBits;
            for (int64_t i = lo + (int)threadIdx.x; i < hi; i += kFairThreads) {
                if (round[i] < 0) continue;
                // rem_b > 0 and rate >= 0: q is positive or +inf, ordered as its bits
                const unsigned long long b =
                    (unsigned long long)__double_as_longlong(ft.remaining[i] / rate[i]);
                bits = b < bits ? b : bits;
            }
            for (int d = SDNR_WAVE / 2; d > 0; d >>= 1) {
                const unsigned long long o = __shfl_xor(bits, d, SDNR_WAVE);
                bits = o < bits ? o : bits;
            }
            if (lane_id() == 0 && bits < kInfBits) atomicMin(&clock->dt[j & 1], bits);
        }
        return;
    }
    ft.j = j;
    ft.dt = j > 0 ? __longlong_as_double((long long)clock->dt[(j - 1) & 1]) : 0.0;
    ft.t = clock->t;
    fair_rows_body<JT, LDS, true>(t, V, E, nextra, nrows, max_steps, clock->round, row_ptr, col,
                                  pair_off, pair_lo, pair_hi, verts, mult, extra, s, rate,
                                  (int32_t *)nullptr, round, scratch, scratch_stride, err,
                                  kErrFairTimes, ft, fair_lds, &s_alive);
}

__global__ __launch_bounds__(kFairLinkThreads) void fair_times_entries_kernel(
    FairState s, FairClock *__restrict__ clock, const double *__restrict__ cap,
    double *__restrict__ carried, double *__restrict__ epoch_time,
    int32_t *__restrict__ epoch_rounds, int n_ent, int nlevel, int max_epochs,
    int *__restrict__ err)
{
    const int phase = clock->phase;
    if (phase >= kPhaseDone) return;                       // the call ended before this step
    const int j = clock->epoch, k = clock->round;
    const unsigned long long dtb = clock->dt[j & 1];
    if (phase == kPhaseFill) {
        fair_links_step(s, n_ent, k);
    } else {
        const int i = (int)(blockIdx.x * (unsigned)kFairLinkThreads + threadIdx.x);
        if (i < n_ent) {
            if (dtb != kInfBits)
                carried[i] = fair_carry(carried[i], s.used[i], __longlong_as_double((long long)dtb));
            s.rem[i] = fair_capacity(cap[i], err, kErrFairTimes);
            s.used[i] = 0.0;
            s.share[i] = __longlong_as_double((long long)kInfBits);
            s.n[i] = 0;
            s.n_prev[i] = 0;
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
                const bool end = __hip_atomic_load(&s.level[k], __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT) == kInfBits;
                if (end && k == 0) {                       // nothing in flight
                    clock->nepochs = j;
                    clock->phase = kPhaseDone;
                } else if (end) {
                    clock->phase = kPhaseAdvance;          // (round stays K_j, the epoch's rounds)
                } else if (k == 0 && j == max_epochs) {
                    clock->nepochs = max_epochs;
                    clock->phase = kPhaseCapped;
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

int sdnr_launch_fair_times(sdnr_ctx *ctx, const void *d_tree, int32_t layout, bool to_root,
                           int32_t nrows, const int64_t *d_pair_off, int64_t pair_lo,
                           int64_t pair_hi, const int32_t *d_verts, const uint64_t *d_mult,
                           const double *d_bytes, const int32_t *d_extra, const double *d_cap,
                           int32_t nextra, double *d_time, int32_t *d_epoch, double *d_rate0,
                           double *d_remaining, double *d_epoch_time, int32_t *d_epoch_rounds,
                           int32_t max_epochs, double *d_carried, int32_t *nepochs)
{
    const int V = ctx->V;
    const int n_ent = ctx->E + nextra;
    const size_t npairs = (size_t)(pair_hi - pair_lo);
    const FairShape shape = fair_shape(ctx, nrows);
    const size_t lds = shape.lds, stride = shape.stride;
    const int64_t g = shape.grid;

    // behind the slices: n, n_prev, rem, share, used, level, alive_row,
    // inflight_row, status, ticket, the clock, then the flows' rate and round
    const size_t max_rounds = npairs < (size_t)n_ent ? npairs : (size_t)n_ent;
    const size_t slices = (stride * (size_t)g + 255) & ~(size_t)255;
    const size_t nlevel = max_rounds + 1;
    const size_t words = 5 * (size_t)n_ent + nlevel + 2 * (size_t)nrows + 2 +
                         sizeof(FairClock) / 8 + npairs + (npairs + 1) / 2;
    const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, slices + 8 * words);
    if (rc) return rc;
    unsigned char *base = static_cast<unsigned char *>(ctx->scratch);
    unsigned long long *w = reinterpret_cast<unsigned long long *>(base + slices);
    FairState s;
    s.n = w;
    s.n_prev = s.n + n_ent;
    s.rem = reinterpret_cast<double *>(s.n_prev + n_ent);
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

    FairRows t{static_cast<const uint32_t *>(d_tree), layout, to_root ? 1 : 0};
    hipStream_t st = ctx->stream;
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, st));
    size_t init_n = (size_t)n_ent > nlevel ? (size_t)n_ent : nlevel;
    if (init_n < npairs) init_n = npairs;
    if (init_n < (size_t)nrows) init_n = (size_t)nrows;
    const size_t ent_n = (size_t)n_ent > nlevel ? (size_t)n_ent : nlevel;
    const unsigned ent_blocks = (unsigned)((ent_n + kFairLinkThreads - 1) / kFairLinkThreads);
    hipLaunchKernelGGL(fair_times_init_kernel,
                       dim3((unsigned)((init_n + kFairLinkThreads - 1) / kFairLinkThreads)),
                       dim3(kFairLinkThreads), 0, st, s, clock, ft, d_cap, d_carried, rate, round,
                       n_ent, (int)nlevel, nrows, pair_lo, pair_hi, ctx->d_err);
    SDNR_HIP(hipGetLastError());
    int launches = 1;
    auto fn_lds = fair_times_rows_kernel<uint16_t, true>;
    if (shape.lds_form) sdnr_allow_lds(reinterpret_cast<const void *>(fn_lds), lds);
    ctx->last_kernel = shape.lds_form ? "fair_times_rows_kernel<lds>" : "fair_times_rows_kernel<global>";
    ctx->last_grid = g;

    // every epoch removes a flow and every round freezes one: more steps than
    // this cannot be needed
    const long long most = ((long long)max_epochs + 1) * ((long long)max_rounds + 2) + 1;
    long long steps = 0;
    int word[4] = {0, 0, 0, 0};
    while (word[0] < kPhaseDone) {
        if (steps > most)
            return sdnr_fail(SDNR_ERR_HIP, "sdnr_fair_times: the clock did not stop in %lld steps",
                             steps);
        for (int b = 0; b < kFairBatch; ++b) {
            if (shape.lds_form)
                hipLaunchKernelGGL(fn_lds, dim3((unsigned)g), dim3(kFairThreads), lds, st, t, V,
                                   ctx->E, nextra, nrows, shape.max_steps, ctx->row_ptr, ctx->col,
                                   d_pair_off, pair_lo, pair_hi, d_verts, d_mult, d_extra, s, clock,
                                   ft, rate, round, (unsigned char *)nullptr, (size_t)0,
                                   ctx->d_err);
            else
                hipLaunchKernelGGL((fair_times_rows_kernel<uint32_t, false>), dim3((unsigned)g),
                                   dim3(kFairThreads), 0, st, t, V, ctx->E, nextra, nrows,
                                   shape.max_steps, ctx->row_ptr, ctx->col, d_pair_off, pair_lo,
                                   pair_hi, d_verts, d_mult, d_extra, s, clock, ft, rate, round,
                                   base, stride, ctx->d_err);
            hipLaunchKernelGGL(fair_times_entries_kernel, dim3(ent_blocks), dim3(kFairLinkThreads),
                               0, st, s, clock, d_cap, d_carried, d_epoch_time, d_epoch_rounds,
                               n_ent, (int)nlevel, max_epochs, ctx->d_err);
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
