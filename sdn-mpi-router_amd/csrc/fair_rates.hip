// fair_rates.hip -- max-min fair flow rates over single-path route tables.
//
// A link load says how much crosses a link; what a rank pair gets follows from
// the loads only through a sharing rule.  Flows on a fabric (TCP, RoCE with
// DCQCN) share bandwidth approximately max-min fairly, and the max-min fair
// allocation is unique: progressive filling finds it.  A flow is a pair of
// sdnr_link_loads (table row r, vertex x) with a multiplicity and up to two
// extra constraints (host ports); its links are the tree links from x to the
// row's root.  With rem = cap, used = 0, n_prev = 0, round k = 0, 1, ...:
//   1. n[e]  = sum of mult over the alive flows crossing e (u64, exact);
//   2. k > 0: m = n_prev[e] - n[e], p = r_{k-1} * (double)m, used[e] += p,
//      rem[e] = max(rem[e] - p, 0)            (each operation rounded alone);
//   3. share[e] = rem[e] / n[e] (n[e] > 0, else +inf), r_k = min share;
//      r_k = +inf: nothing alive crosses anything, stop;
//   4. e is saturated iff share[e] == r_k; every alive flow crossing a
//      saturated link or constraint gets rate r_k, round k and bott = the
//      first saturated tree link from x toward the root, else extra 0, else
//      extra 1, and is dead; n_prev = n.
// Every operation is deterministic (u64 counts, one double operation per link
// and round, a minimum), so the host restatement (engine.fair_rates_host)
// agrees bit for bit.
//
// No grid-wide barrier and no waiting between workgroups: a round is two plain
// launches on the context's stream.
//   fair_rows_kernel (round k), one workgroup per row, persistent over rows:
//     the verdict of round k - 1 and the counts of round k share ONE launch --
//     the verdict only reads share[] / level[k-1] (written by the link kernel
//     before it) and the counts only add into n[] (zeroed by it).
//     Per row visit e_v (the link of v toward the root) is looked up once.
//     (a) verdict: B_0[v] = share[e_v] == r_{k-1} ? e_v : none, J_0 = parent,
//         B_{j+1}[v] = B_j[v] != none ? B_j[v] : B_j[J_j[v]], J_{j+1} = J_j o J_j
//         (gathers only); the row's alive flows read B[x] and their extras'
//         shares and store rate, round, bott.
//     (b) counts: A_0[v] = alive multiplicity at v, subtree sums by the
//         ancestor doubling of loads.hip, one u64 atomic per vertex with a
//         nonzero sum into n[e_v] and one per alive flow's extra.
//     Round 0 classifies the flows instead of (a).  A per-row alive counter
//     lets a row with no alive flow return at once.  Both doublings take
//     ceil(log2(depth + 1)) steps and are bounded by ceil(log2 V) + 1: a row
//     that is no tree sets the error bit, its flows read 0.0 / -1 / -1 and it
//     contributes nothing.  A (two u64 generations), J (two generations, u16)
//     and e_v (i32) live in LDS, 24 bytes per vertex, up to kFairLdsMaxV; B
//     (two i32 generations) aliases A, which (b) fills only after (a) is done.
//     Above that they live in a per-workgroup slice of the context's scratch
//     (u32 ancestors, 28 bytes per vertex), as in loads.hip.
//   fair_links_kernel (round k), over the E + nextra entries: step 2, share,
//     n_prev = n, n = 0, a wave-reduced minimum into level[k] (atomicMin on the
//     bits: non-negative doubles order as their bit patterns), and the last
//     workgroup to finish stores k + 1 into the status word if level[k] is
//     +inf.  A kernel launched after that sees the status and returns.
// The host queues kFairBatch rounds, reads the 8-byte status word back, and
// goes on until it is set (or max_rounds rounds were run).
#include "fair_rows.h"

#include <string.h>

namespace {

__global__ __launch_bounds__(kFairLinkThreads) void fair_init_kernel(
    FairState s, const double *__restrict__ cap, int n_ent, int nlevel, int *__restrict__ err)
{
    const int i = (int)(blockIdx.x * (unsigned)kFairLinkThreads + threadIdx.x);
    if (i < n_ent) {
        double c = cap[i];
        if (!(c > 0.0) || __double_as_longlong(c) == (long long)kInfBits) {
            atomicOr(err, kErrFairRates);                  // not positive and finite
            c = __longlong_as_double((long long)kInfBits); // (never saturates: results invalid)
        }
        s.rem[i] = c;
        s.used[i] = 0.0;
        s.share[i] = __longlong_as_double((long long)kInfBits);
        s.n[i] = 0;
        s.n_prev[i] = 0;
    }
    if (i < nlevel) s.level[i] = kInfBits;
    if (i == 0) {
        *s.status = 0;
        *s.ticket = 0;
    }
}

// JT: u16 (LDS, none 0xFFFF) or u32 (global scratch, none 0xFFFFFFFF); the
// body is fair_rows.h's, which sdnr_fair_times runs too
template <typename JT, bool LDS>
__global__ __launch_bounds__(kFairThreads) void fair_rows_kernel(
    FairRows t, int V, int E, int nextra, int nrows, int max_steps, int k,
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int64_t *__restrict__ pair_off, int64_t pair_lo, int64_t pair_hi,
    const int32_t *__restrict__ verts, const uint64_t *__restrict__ mult,
    const int32_t *__restrict__ extra, FairState s, double *__restrict__ rate,
    int32_t *__restrict__ bott, int32_t *__restrict__ round, unsigned char *__restrict__ scratch,
    size_t scratch_stride, int *__restrict__ err)
{
    extern __shared__ unsigned long long fair_lds[];
    __shared__ unsigned long long s_alive;
    if (k > 0 && *s.status) return;                        // the rounds ended before this one
    fair_rows_body<JT, LDS, false>(t, V, E, nextra, nrows, max_steps, k, row_ptr, col, pair_off,
                                   pair_lo, pair_hi, verts, mult, extra, s, rate, bott, round,
                                   scratch, scratch_stride, err, kErrFairRates, FairTimes{},
                                   fair_lds, &s_alive);
}

__global__ __launch_bounds__(kFairLinkThreads) void fair_links_kernel(FairState s, int n_ent, int k)
{
    if (k > 0 && *s.status) return;                        // the rounds ended before this one
    fair_links_step(s, n_ent, k);
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(s.ticket, 1u) == gridDim.x - 1) {    // the last workgroup of the pass
            __threadfence();
            *s.ticket = 0;
            if (__hip_atomic_load(&s.level[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                kInfBits)
                *s.status = (unsigned long long)k + 1;
        }
    }
}

}  // namespace

int sdnr_launch_fair_rates(sdnr_ctx *ctx, const void *d_tree, int32_t layout, bool to_root,
                           int32_t nrows, const int64_t *d_pair_off, int64_t pair_lo,
                           int64_t pair_hi, const int32_t *d_verts, const uint64_t *d_mult,
                           const int32_t *d_extra, const double *d_cap, int32_t nextra,
                           double *d_rate, int32_t *d_bott, int32_t *d_round, double *d_level,
                           int32_t max_rounds, double *d_used, int32_t *nrounds)
{
    const int V = ctx->V;
    const int n_ent = ctx->E + nextra;
    const size_t npairs = (size_t)(pair_hi - pair_lo);

    // the row kernel's shape, and its per-workgroup scratch slices
    const FairShape shape = fair_shape(ctx, nrows);
    const bool lds_form = shape.lds_form;
    const size_t lds = shape.lds, stride = shape.stride;
    const int64_t g = shape.grid;
    const int max_steps = shape.max_steps;

    // the state behind the slices: n, n_prev, rem, share, level, alive_row, status, ticket
    const size_t slices = (stride * (size_t)g + 255) & ~(size_t)255;
    const size_t nlevel = (size_t)max_rounds + 1;
    const size_t state = 8 * (4 * (size_t)n_ent + nlevel + (size_t)nrows + 2);
    const int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, slices + state);
    if (rc) return rc;
    unsigned char *base = static_cast<unsigned char *>(ctx->scratch);
    unsigned long long *w = reinterpret_cast<unsigned long long *>(base + slices);
    FairState s;
    s.n = w;
    s.n_prev = s.n + n_ent;
    s.rem = reinterpret_cast<double *>(s.n_prev + n_ent);
    s.share = s.rem + n_ent;
    s.level = reinterpret_cast<unsigned long long *>(s.share + n_ent);
    s.alive_row = reinterpret_cast<long long *>(s.level + nlevel);
    s.status = reinterpret_cast<unsigned long long *>(s.alive_row + nrows);
    s.ticket = reinterpret_cast<unsigned int *>(s.status + 1);
    s.used = d_used;

    FairRows t{static_cast<const uint32_t *>(d_tree), layout, to_root ? 1 : 0};
    hipStream_t st = ctx->stream;
    // every flow reads 0.0 / -1 / -1 until a row says otherwise
    SDNR_HIP(hipMemsetAsync(d_rate + pair_lo, 0, npairs * sizeof(double), st));
    SDNR_HIP(hipMemsetAsync(d_bott + pair_lo, 0xFF, npairs * sizeof(int32_t), st));
    SDNR_HIP(hipMemsetAsync(d_round + pair_lo, 0xFF, npairs * sizeof(int32_t), st));
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, st));
    const size_t init_n = (size_t)n_ent > nlevel ? (size_t)n_ent : nlevel;
    unsigned link_blocks = (unsigned)((n_ent + kFairLinkThreads - 1) / kFairLinkThreads);
    if (link_blocks == 0) link_blocks = 1;                 // (no link, no extra: level[0] = +inf)
    hipLaunchKernelGGL(fair_init_kernel,
                       dim3((unsigned)((init_n + kFairLinkThreads - 1) / kFairLinkThreads)),
                       dim3(kFairLinkThreads), 0, st, s, d_cap, n_ent, (int)nlevel, ctx->d_err);
    SDNR_HIP(hipGetLastError());
    int launches = 1;
    auto fn_lds = fair_rows_kernel<uint16_t, true>;
    if (lds_form) sdnr_allow_lds(reinterpret_cast<const void *>(fn_lds), lds);
    ctx->last_kernel = lds_form ? "fair_rows_kernel<lds>" : "fair_rows_kernel<global>";
    ctx->last_grid = g;

    int k = 0, done = -1;
    while (done < 0) {
        // rounds 0 .. max_rounds: the last one only applies the verdict of
        // round max_rounds - 1 and makes used final
        const int end = k + kFairBatch <= max_rounds + 1 ? k + kFairBatch : max_rounds + 1;
        for (; k < end; ++k) {
            if (lds_form)
                hipLaunchKernelGGL(fn_lds, dim3((unsigned)g), dim3(kFairThreads), lds, st, t, V,
                                   ctx->E, nextra, nrows, max_steps, k, ctx->row_ptr, ctx->col,
                                   d_pair_off, pair_lo, pair_hi, d_verts, d_mult, d_extra, s,
                                   d_rate, d_bott, d_round, (unsigned char *)nullptr, (size_t)0,
                                   ctx->d_err);
            else
                hipLaunchKernelGGL((fair_rows_kernel<uint32_t, false>), dim3((unsigned)g),
                                   dim3(kFairThreads), 0, st, t, V, ctx->E, nextra, nrows,
                                   max_steps, k, ctx->row_ptr, ctx->col, d_pair_off, pair_lo,
                                   pair_hi, d_verts, d_mult, d_extra, s, d_rate, d_bott, d_round,
                                   base, stride, ctx->d_err);
            hipLaunchKernelGGL(fair_links_kernel, dim3(link_blocks), dim3(kFairLinkThreads), 0, st,
                               s, n_ent, k);
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
