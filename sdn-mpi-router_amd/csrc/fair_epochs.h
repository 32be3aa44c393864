// fair_epochs.h -- what the single-path (fair_rows.h) and the multipath
// (ecmp_fair_rows.h) fair-sharing kernels have in common: the batch and round
// constants, the capacity rule, and what the completion-time calls
// (fair_times.hip, ecmp_fair_times.hip) add to a filling -- the flows' byte
// state, the clock in device memory and the arithmetic of the advance.
#ifndef SDNR_FAIR_EPOCHS_H
#define SDNR_FAIR_EPOCHS_H

#include "common.h"

namespace {

constexpr int kFairBatch = 16;           // rounds queued per status read-back
constexpr int kFairAlive = -2;           // round[] of a flow not frozen yet
constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;

// TIMES: what a flow of sdnr_fair_times carries beside its rate and round.
// round[] there is kFairAlive (in flight, not frozen in this epoch's filling),
// >= 0 (in flight, frozen) or -1 (not in flight: absent, at the root, without
// bytes, or finished).
struct FairTimes {
    const double *bytes;          // [npairs] the caller's
    double *remaining;            // [npairs] rem_b, the caller's
    double *time;                 // [npairs] the caller's, preset +inf
    int32_t *epoch;               // [npairs] the caller's, preset -1
    double *rate0;                // [npairs] the caller's, preset 0.0
    long long *inflight_row;      // [nrows] flows of a row in flight
    int j;                        // the running epoch
    int max_epochs;
    double dt;                    // j > 0: what epoch j - 1 lasted
    double t;                     // j > 0: t_{j-1}
};

// TIMES: the clock of a completion-time call (fair_times.hip,
// ecmp_fair_times.hip), in device memory; only the last workgroup of an entry
// pass moves it
constexpr int kPhaseFill = 0, kPhaseAdvance = 1, kPhaseDone = 2, kPhaseCapped = 3;

struct FairClock {
    int phase, epoch, round, nepochs;   // (the four words the host reads)
    double t;                           // t_{epoch - 1}
    unsigned long long dt[2];           // bits of dt of epoch j in dt[j & 1], +inf until it ran
};

// TIMES: carried + used * dt, the multiply and the add rounded one by one
__device__ __forceinline__ double fair_carry(double carried, double used, double dt)
{
#pragma clang fp contract(off)
    const double sent = used * dt;
    return carried + sent;
}

// a capacity as the filling takes it: +inf (never saturates) and the error bit
// for one that is not positive and finite
__device__ __forceinline__ double fair_capacity(double c, int *__restrict__ err, int bit)
{
    if (!(c > 0.0) || __double_as_longlong(c) == (long long)kInfBits) {
        atomicOr(err, bit);
        c = __longlong_as_double((long long)kInfBits);
    }
    return c;
}

// TIMES: rem_b - rate * dt, the multiply and the subtract rounded one by one
__device__ __forceinline__ double fair_bytes_left(double rem_b, double rate, double dt)
{
#pragma clang fp contract(off)
    const double sent = rate * dt;
    return rem_b - sent;
}

}  // namespace

#endif  // SDNR_FAIR_EPOCHS_H
