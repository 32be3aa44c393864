// frr_loads.hip -- fast-reroute what-if loads: what every link carries while
// the switches' loop-free-alternate backup buckets are forwarding, once per
// failure scenario, before the controller has re-routed anything.
//
// Forwarding toward d = dst[r] in scenario k, from the least-cost next hops
// nh[r] and the backups backup[r] (lfa_tables.hip), both taken as given:
//   fwd(x) = nh[x]      if the link x -> nh[x] is not in the scenario,
//          = backup[x]  if it is, a backup exists and the link x -> backup[x]
//                       is not in the scenario (a REPAIR),
//          = nothing    otherwise (x DROPS); a switch without nh[x] forwards
//                       nowhere in any scenario, and d itself forwards nowhere
//                       (its own entries are not read).
// A pair (s, d) follows fwd from s: status 0 no base route (following nh alone
// does not end at d) or s outside [0, V); 1 delivered over primaries only (s ==
// d included); 2 delivered through at least one repair; 3 dropped, the walk
// ends at a switch other than d; 4 looped, the walk never ends.  Only delivered
// pairs add load: their weight on every link of their walk.  u64 sums that
// wrap, so the order of the atomics does not matter.
//
// A failed link x -> n changes the forwarding toward d only if nh[x] == n, so
// of the nscen x nrows (scenario, row) items only a few differ from the base --
// one per (destination, switch with a primary) over a single-link sweep.  The
// call therefore runs
//   1. entries  per scenario entry its link's ends (x by bisection in row_ptr)
//               and its scenario; the order check: a scenario that does not
//               ascend is reported and taken as empty;
//   2. base     per row, one workgroup: the row without any failure.  Subtree
//               sums of the routed sources over nh (loads.hip's ancestor
//               doubling) go to Tbase[r][V] and, per link, to base[E] in the
//               context scratch, with the base status (0 / 1) of every pair;
//               the row is checked here (an in-tree of the graph);
//   3. affected the items (k, r) where some entry of scenario k has
//               nh[r][x] == n, each listed once (a bit per item);
//   4. spread   load[k] += base, status[k] = base status, stat[k][3] += the
//               weight without a base route: one streaming pass;
//   5. items    one workgroup per AFFECTED item, persistent over the list, the
//               row's state in LDS: patch fwd, classify every vertex by
//               pointer jumping, sum the delivered sources over the patched
//               forest, and for every vertex whose link or sum differs from
//               Tbase issue load[k][e_base] -= Tb, load[k][e_new] += T';
//   6. peak     the largest entry of every plane as it stands then.
// An unaffected item costs its test in step 3 and nothing else.
//
// Classification.  word[x] = J | repair << 16 | end << 17: J an ancestor of x
// under fwd, repair the OR of "x' repairs" over the walk x .. J (J excluded),
// end != 0 once the walk's end is known (the end's kind).  A vertex that
// forwards nowhere is its own J with its kind set from the start.  A round
// replaces word[x] by (J of word[J], the flags of both): one 32-bit LDS word
// per vertex, read and written whole, so the rounds run in place -- whatever
// mix of old and new words a thread reads, each is a true statement about the
// walk.  After round t a vertex knows its end or has a J at least 2^t links
// ahead, so ceil(log2 V) + 1 rounds settle every walk that ends; what has no
// end by then is on or behind a cycle.
//
// Row state: two u64 and two u16 generations of the doubling (loads.hip), the
// u32 word and the u16 patched next hop: 26 bytes per vertex, V <= kFrrMaxV.
#include "common.h"

namespace {

constexpr int kFrrThreads = 512;
constexpr int kPeakThreads = 256;
constexpr uint32_t kJMask = 0xFFFFu;
constexpr uint32_t kRepair = 1u << 16;
constexpr int kEndShift = 17;
// how a walk ends: at d, at a switch without a base route, at a switch that
// drops, in a self-loop backup
constexpr uint32_t kEndDst = 1, kEndNone = 2, kEndDrop = 3, kEndSelf = 4;
constexpr uint16_t kNoHop = 0xFFFF;

struct FrrScratch {
    unsigned long long *base;      // [E] base loads
    unsigned long long *ctr;       // [0] affected items, [1] weight without a base route
    uint8_t *rowinfo;              // [nrows] 1: the row has pairs and passed its checks
    uint8_t *bstat;                // [npairs] base status
    uint32_t *bits;                // one bit per item: listed
    int32_t *ex, *en, *ek;         // per scenario entry: link x -> n, scenario (x -1: ignored)
    long long *list;               // the affected items, k * nrows + r
    unsigned long long *tbase;     // [nrows][V] base subtree sums
};

struct FrrLds {
    unsigned long long *A;         // [2][V]
    uint32_t *word;                // [V]
    uint16_t *J;                   // [2][V]
    uint16_t *fwd;                 // [V]
};

__device__ __forceinline__ FrrLds frr_lds(unsigned char *p, int V)
{
    FrrLds s;
    s.A = reinterpret_cast<unsigned long long *>(p);
    s.word = reinterpret_cast<uint32_t *>(s.A + 2 * (size_t)V);
    s.J = reinterpret_cast<uint16_t *>(s.word + V);
    s.fwd = s.J + 2 * (size_t)V;
    return s;
}

__device__ __forceinline__ uint32_t word_ld(const uint32_t *w)
{
    return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void word_st(uint32_t *w, uint32_t v)
{
    __hip_atomic_store(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// word[] and fwd[] of the row without failures.  Returns false where an entry
// names no vertex or the vertex itself.
__device__ __forceinline__ bool frr_init_row(const FrrLds &s, const int32_t *__restrict__ nh, int d,
                                             int V)
{
    bool ok = true;
    for (int x = (int)threadIdx.x; x < V; x += kFrrThreads) {
        const int p = x == d ? -1 : nh[x];
        uint32_t w;
        if (x == d) {
            w = (uint32_t)x | kEndDst << kEndShift;
        } else if (p < 0) {
            w = (uint32_t)x | kEndNone << kEndShift;
        } else if (p >= V || p == x) {
            ok = false;
            w = (uint32_t)x | kEndNone << kEndShift;
        } else {
            w = (uint32_t)p;
        }
        s.word[x] = w;
        s.fwd[x] = (w >> kEndShift) ? kNoHop : (uint16_t)p;
    }
    return ok;
}

// the rounds of the classification; ends with every thread past a barrier
__device__ __forceinline__ void frr_jump(uint32_t *word, int V, int max_rounds)
{
    for (int round = 0; round < max_rounds; ++round) {
        int changed = 0;
        for (int x = (int)threadIdx.x; x < V; x += kFrrThreads) {
            const uint32_t w = word_ld(&word[x]);
            if (w >> kEndShift) continue;
            const uint32_t wj = word_ld(&word[w & kJMask]);
            const uint32_t nw = (wj & kJMask) | ((w | wj) & ~kJMask);
            if (nw != w) {
                word_st(&word[x], nw);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) return;
    }
}

// loads.hip's ancestor doubling over generation 0 of A and J (filled, a
// barrier passed; more: some J is valid).  Returns the generation that holds
// the subtree sums, NULL if the chains outran max_rounds (uniform).
__device__ __forceinline__ const unsigned long long *frr_sums(const FrrLds &s, int V, int more,
                                                              int max_rounds)
{
    const int tid = (int)threadIdx.x;
    int cur = 0, rounds = 0;
    while (more) {
        if (rounds == max_rounds) return nullptr;
        unsigned long long *Ac = s.A + (cur ? V : 0), *An = s.A + (cur ? 0 : V);
        uint16_t *Jc = s.J + (cur ? V : 0), *Jn = s.J + (cur ? 0 : V);
        for (int v = tid; v < V; v += kFrrThreads) An[v] = Ac[v];
        __syncthreads();
        int any = 0;
        for (int v = tid; v < V; v += kFrrThreads) {
            const uint16_t j = Jc[v];
            uint16_t jj = kNoHop;
            if (j != kNoHop) {
                const unsigned long long a = Ac[v];
                if (a) atomicAdd(&An[j], a);
                jj = Jc[j];
                any |= jj != kNoHop;
            }
            Jn[v] = jj;
        }
        more = __syncthreads_or(any);
        cur ^= 1;
        ++rounds;
    }
    return s.A + (cur ? V : 0);
}

// 1. one workgroup per scenario, persistent
__global__ __launch_bounds__(256) void frr_entries_kernel(
    int V, int E, int nscen, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int64_t *__restrict__ scen_off, int64_t scen_lo, int64_t scen_hi,
    const int32_t *__restrict__ scen_edges, FrrScratch q, int *__restrict__ err)
{
    const int tid = (int)threadIdx.x;
    for (int k = (int)blockIdx.x; k < nscen; k += (int)gridDim.x) {
        const int64_t lo = scen_off[k], hi = scen_off[k + 1];
        if (lo < scen_lo || hi > scen_hi || hi < lo ||
            hi - lo > (int64_t)0x7FFFFFF0) {               // offsets outside the scenario list
            if (tid == 0) atomicOr(err, kErrFrrLoads);
            continue;
        }
        int disorder = 0;
        for (int64_t i = lo + 1 + tid; i < hi; i += 256)
            disorder |= scen_edges[i - 1] > scen_edges[i];
        if (__syncthreads_or(disorder)) {                  // taken as empty: x stays -1
            if (tid == 0) atomicOr(err, kErrFrrLoads);
            continue;
        }
        for (int64_t i = lo + tid; i < hi; i += 256) {
            const int f = scen_edges[i];
            if (f < 0 || f >= E) {                         // no link: ignored, reported
                atomicOr(err, kErrFrrLoads);
                continue;
            }
            int a = 0, b = V;                              // the x with row_ptr[x] <= f < row_ptr[x + 1]
            while (b - a > 1) {
                const int m = a + ((b - a) >> 1);
                if (row_ptr[m] <= f) a = m;
                else b = m;
            }
            q.ex[i - scen_lo] = a;
            q.en[i - scen_lo] = col[f];
            q.ek[i - scen_lo] = k;
        }
    }
}

// 2. one workgroup per row, persistent
__global__ __launch_bounds__(kFrrThreads) void frr_base_kernel(
    int V, int nrows, int max_rounds, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const int32_t *__restrict__ dst,
    const int32_t *__restrict__ nh, const int64_t *__restrict__ pair_off, int64_t pair_lo,
    int64_t pair_hi, const int32_t *__restrict__ srcs, const uint64_t *__restrict__ weight,
    FrrScratch q, int *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char frr_base_lds[];
    const FrrLds s = frr_lds(frr_base_lds, V);
    const int tid = (int)threadIdx.x;

    for (int r = (int)blockIdx.x; r < nrows; r += (int)gridDim.x) {
        const int64_t lo = pair_off[r], hi = pair_off[r + 1];
        if (lo < pair_lo || hi > pair_hi || hi < lo) {     // offsets outside the pair list
            if (tid == 0) atomicOr(err, kErrFrrLoads);
            continue;
        }
        if (lo == hi) continue;                            // (uniform: the row has no demand)
        const int d = dst[r];
        if (d < 0 || d >= V) {                             // (uniform) no vertex: nothing routed
            unsigned long long gone = 0;
            for (int64_t i = lo + tid; i < hi; i += kFrrThreads) gone += weight ? weight[i] : 1ull;
            if (gone) atomicAdd(&q.ctr[1], gone);
            continue;
        }
        const int32_t *nhr = nh + (size_t)r * (size_t)V;
        __syncthreads();                                   // the previous row is done with the LDS
        int bad = frr_init_row(s, nhr, d, V) ? 0 : 1;
        if (__syncthreads_or(bad)) {
            if (tid == 0) atomicOr(err, kErrFrrLoads);
            continue;
        }
        frr_jump(s.word, V, max_rounds);
        // a walk without an end: nh has a cycle
        int any0 = 0;
        for (int x = tid; x < V; x += kFrrThreads) {
            const uint32_t end = s.word[x] >> kEndShift;
            bad |= end == 0;
            s.A[x] = 0;
            const uint16_t j = (end == kEndDst && x != d) ? s.fwd[x] : kNoHop;
            s.J[x] = j;
            any0 |= j != kNoHop;
        }
        const int more = __syncthreads_or(any0);
        for (int64_t i = lo + tid; i < hi; i += kFrrThreads) {
            const int src = srcs[i];
            if (src < 0 || src >= V || (s.word[src] >> kEndShift) != kEndDst) continue;
            const unsigned long long w = weight ? (unsigned long long)weight[i] : 1ull;
            if (w) atomicAdd(&s.A[src], w);
        }
        __syncthreads();
        const unsigned long long *T = frr_sums(s, V, more, max_rounds);
        if (!T) bad = 1;
        // every link that carries something is a link of the graph
        for (int x = tid; T && x < V; x += kFrrThreads) {
            if (x == d || !T[x] || s.fwd[x] == kNoHop) continue;
            if (edge_index(row_ptr, col, x, (int)s.fwd[x]) < 0) bad = 1;
        }
        if (__syncthreads_or(bad)) {
            if (tid == 0) atomicOr(err, kErrFrrLoads);
            continue;
        }
        unsigned long long *tb = q.tbase + (size_t)r * (size_t)V;
        for (int x = tid; x < V; x += kFrrThreads) {
            const unsigned long long t = (x == d || s.fwd[x] == kNoHop) ? 0ull : T[x];
            tb[x] = t;
            if (t) atomicAdd(&q.base[edge_index(row_ptr, col, x, (int)s.fwd[x])], t);
        }
        unsigned long long gone = 0;
        for (int64_t i = lo + tid; i < hi; i += kFrrThreads) {
            const int src = srcs[i];
            const bool ok = src >= 0 && src < V && (s.word[src] >> kEndShift) == kEndDst;
            q.bstat[i - pair_lo] = ok ? 1 : 0;
            if (!ok) gone += weight ? weight[i] : 1ull;
        }
        if (gone) atomicAdd(&q.ctr[1], gone);
        if (tid == 0) q.rowinfo[r] = 1;
    }
}

// 3. blockIdx.x strides the rows, blockIdx.y the scenario entries
__global__ __launch_bounds__(256) void frr_affected_kernel(
    int V, int nrows, int64_t nent, const int32_t *__restrict__ dst,
    const int32_t *__restrict__ nh, FrrScratch q)
{
    for (int r = (int)blockIdx.x; r < nrows; r += (int)gridDim.x) {
        if (!q.rowinfo[r]) continue;
        const int d = dst[r];
        const int32_t *nhr = nh + (size_t)r * (size_t)V;
        for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < nent;
             i += (int64_t)gridDim.y * 256) {
            const int x = q.ex[i];
            if (x < 0 || x == d || nhr[x] != q.en[i]) continue;
            const long long item = (long long)q.ek[i] * nrows + r;
            const uint32_t m = 1u << (item & 31);
            if (atomicOr(&q.bits[item >> 5], m) & m) continue;     // listed already
            q.list[atomicAdd(&q.ctr[0], 1ull)] = item;
        }
    }
}

// 4. blockIdx.y strides the scenarios
__global__ __launch_bounds__(256) void frr_spread_kernel(
    int E, int nscen, int64_t npairs, FrrScratch q, unsigned long long *__restrict__ load,
    unsigned long long *__restrict__ stat, unsigned char *__restrict__ status)
{
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int k = (int)blockIdx.y; k < nscen; k += (int)gridDim.y) {
        unsigned long long *out = load + (size_t)k * (size_t)E;
        for (int64_t e = t0; e < E; e += step) {
            const unsigned long long b = q.base[e];
            if (b) out[e] += b;
        }
        if (status) {
            unsigned char *st = status + (size_t)k * (size_t)npairs;
            for (int64_t i = t0; i < npairs; i += step) st[i] = q.bstat[i];
        }
        if (stat && t0 == 0 && q.ctr[1]) stat[(size_t)k * 4 + 3] += q.ctr[1];
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int s = SDNR_WAVE / 2; s >= 1; s >>= 1) v += __shfl_down(v, s);
    return v;
}

// 5. one workgroup per affected item, persistent over the list
__global__ __launch_bounds__(kFrrThreads) void frr_items_kernel(
    int V, int E, int nrows, int max_rounds, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const int32_t *__restrict__ dst,
    const int32_t *__restrict__ nh, const int32_t *__restrict__ backup,
    const int64_t *__restrict__ pair_off, int64_t pair_lo, const int32_t *__restrict__ srcs,
    const uint64_t *__restrict__ weight, const int64_t *__restrict__ scen_off, int64_t scen_lo,
    FrrScratch q, unsigned long long *__restrict__ load, unsigned long long *__restrict__ stat,
    unsigned char *__restrict__ status, int64_t npairs, int *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char frr_item_lds[];
    const FrrLds s = frr_lds(frr_item_lds, V);
    const int tid = (int)threadIdx.x;
    const long long nitems = (long long)q.ctr[0];

    for (long long it = (long long)blockIdx.x; it < nitems; it += (long long)gridDim.x) {
        const long long item = q.list[it];
        const int k = (int)(item / nrows), r = (int)(item % nrows);
        // (a listed item: its row and its scenario passed steps 1 and 2)
        const int64_t lo = pair_off[r], hi = pair_off[r + 1];
        const int64_t flo = scen_off[k] - scen_lo;
        const int nent = (int)(scen_off[k + 1] - scen_off[k]);
        const int d = dst[r];
        const int32_t *nhr = nh + (size_t)r * (size_t)V;
        const int32_t *bkr = backup + (size_t)r * (size_t)V;
        const int32_t *ex = q.ex + flo, *en = q.en + flo;

        __syncthreads();                                   // the previous item is done with the LDS
        frr_init_row(s, nhr, d, V);
        __syncthreads();
        // the scenario's links that are primaries: repair or drop
        int bad = 0;
        for (int i = tid; i < nent; i += kFrrThreads) {
            const int x = ex[i];
            if (x < 0 || x == d || nhr[x] != en[i]) continue;
            const int b = bkr[x];
            bool drop = true;
            if (b >= V || b < -1) {
                bad = 1;                                   // no vertex
            } else if (b >= 0) {
                if (edge_index(row_ptr, col, x, b) < 0) {
                    bad = 1;                               // no out-neighbour
                } else {
                    // the entries of x are neighbours in the list: it ascends
                    bool dead = b == en[i];                // (a backup that is the primary)
                    for (int j = i - 1; j >= 0 && ex[j] == x; --j) dead |= en[j] == b;
                    for (int j = i + 1; j < nent && ex[j] == x; ++j) dead |= en[j] == b;
                    drop = dead;
                }
            }
            // (duplicates of the entry write the same words)
            if (drop) {
                s.word[x] = (uint32_t)x | kEndDrop << kEndShift;
                s.fwd[x] = kNoHop;
            } else if (b == x) {
                s.word[x] = (uint32_t)x | kEndSelf << kEndShift;
                s.fwd[x] = kNoHop;
            } else {
                s.word[x] = (uint32_t)b | kRepair;
                s.fwd[x] = (uint16_t)b;
            }
        }
        if (__syncthreads_or(bad)) {                       // the item adds nothing: the base stands
            if (tid == 0) atomicOr(err, kErrFrrLoads);
            continue;
        }
        frr_jump(s.word, V, max_rounds);

        int any0 = 0;
        for (int x = tid; x < V; x += kFrrThreads) {
            s.A[x] = 0;
            const uint16_t j = ((s.word[x] >> kEndShift) == kEndDst && x != d) ? s.fwd[x] : kNoHop;
            s.J[x] = j;
            any0 |= j != kNoHop;
        }
        const int more = __syncthreads_or(any0);
        unsigned long long sum2 = 0, sum3 = 0, sum4 = 0;
        unsigned char *st = status ? status + (size_t)k * (size_t)npairs : nullptr;
        for (int64_t i = lo + tid; i < hi; i += kFrrThreads) {
            if (!q.bstat[i - pair_lo]) continue;           // no base route: 0 stands
            const int src = srcs[i];
            const uint32_t w32 = s.word[src];
            const uint32_t end = w32 >> kEndShift;
            const unsigned long long w = weight ? (unsigned long long)weight[i] : 1ull;
            int code;
            if (end == kEndDst) {
                code = (w32 & kRepair) ? 2 : 1;
                if (w) atomicAdd(&s.A[src], w);
                if (code == 2) sum2 += w;
            } else if (end == kEndNone || end == kEndDrop) {
                code = 3;
                sum3 += w;
            } else {
                code = 4;
                sum4 += w;
            }
            if (st) st[i - pair_lo] = (unsigned char)code;
        }
        if (stat) {
            sum2 = wave_sum(sum2);
            sum3 = wave_sum(sum3);
            sum4 = wave_sum(sum4);
            if ((tid & (SDNR_WAVE - 1)) == 0) {
                unsigned long long *o = stat + (size_t)k * 4;
                if (sum2) atomicAdd(&o[0], sum2);
                if (sum3) atomicAdd(&o[1], sum3);
                if (sum4) atomicAdd(&o[2], sum4);
            }
        }
        __syncthreads();
        const unsigned long long *T = frr_sums(s, V, more, max_rounds);
        if (!T) {                                          // (a forest of V vertices cannot)
            if (tid == 0) atomicOr(err, kErrFrrLoads);
            continue;
        }

        // the links whose load differs from the base
        unsigned long long *out = load + (size_t)k * (size_t)E;
        const unsigned long long *tb = q.tbase + (size_t)r * (size_t)V;
        for (int x = tid; x < V; x += kFrrThreads) {
            if (x == d) continue;
            const unsigned long long b0 = tb[x];
            const int np = s.fwd[x] == kNoHop ? -1 : (int)s.fwd[x];
            const unsigned long long t1 = np < 0 ? 0ull : T[x];
            if (!b0 && !t1) continue;
            const int nb = nhr[x];
            if (nb == np) {
                if (t1 == b0) continue;
                const int e = edge_index(row_ptr, col, x, nb);
                if (e >= 0) atomicAdd(&out[e], t1 - b0);
                continue;
            }
            if (b0) {
                const int e = edge_index(row_ptr, col, x, nb);
                if (e >= 0) atomicAdd(&out[e], 0ull - b0);
            }
            if (t1) {
                const int e = edge_index(row_ptr, col, x, np);
                if (e >= 0) atomicAdd(&out[e], t1);
            }
        }
    }
}

// 6. peak[k] = max over e of load[k][e], peak_edge[k] = the smallest e that
// attains it; 0 and -1 when no link carries anything
__global__ __launch_bounds__(kPeakThreads) void frr_peak_kernel(
    int E, int nscen, const unsigned long long *__restrict__ load,
    unsigned long long *__restrict__ peak, int32_t *__restrict__ peak_edge)
{
    __shared__ unsigned long long wave_u[kPeakThreads / SDNR_WAVE];
    __shared__ int wave_e[kPeakThreads / SDNR_WAVE];
    const int tid = (int)threadIdx.x;
    for (int k = (int)blockIdx.x; k < nscen; k += (int)gridDim.x) {
        const unsigned long long *row = load + (size_t)k * (size_t)E;
        unsigned long long bu = 0;
        int be = -1;
        for (int e = tid; e < E; e += kPeakThreads) {      // e ascends: a tie keeps the first
            const unsigned long long u = row[e];
            if (u > bu) {
                bu = u;
                be = e;
            }
        }
        // (be == -1 goes with bu == 0 and only then)
        for (int s = SDNR_WAVE / 2; s >= 1; s >>= 1) {
            const unsigned long long ou = __shfl_down(bu, s);
            const int oe = __shfl_down(be, s);
            if (oe >= 0 && (ou > bu || (ou == bu && oe < be))) {
                bu = ou;
                be = oe;
            }
        }
        if ((tid & (SDNR_WAVE - 1)) == 0) {
            wave_u[tid / SDNR_WAVE] = bu;
            wave_e[tid / SDNR_WAVE] = be;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kPeakThreads / SDNR_WAVE; ++w)
                if (wave_e[w] >= 0 && (wave_u[w] > bu || (wave_u[w] == bu && wave_e[w] < be))) {
                    bu = wave_u[w];
                    be = wave_e[w];
                }
            peak[k] = bu;
            peak_edge[k] = be;
        }
        __syncthreads();                                   // the wave words are reused
    }
}

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

int sdnr_launch_frr_link_loads(sdnr_ctx *ctx, const int32_t *d_dst, const int32_t *d_nh,
                               const int32_t *d_backup, int32_t nrows, const int64_t *d_pair_off,
                               int64_t pair_lo, int64_t pair_hi, const int32_t *d_srcs,
                               const uint64_t *d_weight, int32_t nscen,
                               const int64_t *d_scen_off, int64_t scen_lo, int64_t scen_hi,
                               const int32_t *d_scen_edges, uint64_t *d_load, uint64_t *d_stat,
                               uint8_t *d_status)
{
    const int V = ctx->V, E = ctx->E;
    const int64_t npairs = pair_hi - pair_lo, nent = scen_hi - scen_lo;
    const int64_t nitems = (int64_t)nscen * (int64_t)nrows;
    int max_rounds = 1;                                    // ceil(log2 V) + 1
    while ((1ll << (max_rounds - 1)) < (long long)V) ++max_rounds;

    // the scratch: what is zeroed first, then the entry ends (x = -1), then the rest
    const size_t o_base = 0;
    const size_t o_ctr = o_base + up256((size_t)E * 8);
    const size_t o_rowinfo = o_ctr + 256;
    const size_t o_bstat = o_rowinfo + up256((size_t)nrows);
    const size_t o_bits = o_bstat + up256((size_t)npairs);
    const size_t o_ex = o_bits + up256((size_t)((nitems + 31) / 32) * 4);
    const size_t o_en = o_ex + up256((size_t)nent * 4);
    const size_t o_ek = o_en + up256((size_t)nent * 4);
    const size_t o_list = o_ek + up256((size_t)nent * 4);
    const size_t o_tbase = o_list + up256((size_t)nitems * 8);
    const size_t total = o_tbase + up256((size_t)nrows * (size_t)V * 8);
    if (total > kLoadsScratchBytes)
        return sdnr_fail(SDNR_ERR_NOMEM, "sdnr_frr_link_loads: %zu bytes of scratch for %d "
                         "scenarios x %d rows exceed %zu (split the scenarios)", total, nscen,
                         nrows, kLoadsScratchBytes);
    int rc = sdnr_reserve(&ctx->scratch, &ctx->scratch_bytes, total);
    if (rc) return rc;
    if (!ctx->h_frr_items)
        SDNR_HIP(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_frr_items), sizeof(int64_t)));
    unsigned char *sb = static_cast<unsigned char *>(ctx->scratch);
    FrrScratch q;
    q.base = reinterpret_cast<unsigned long long *>(sb + o_base);
    q.ctr = reinterpret_cast<unsigned long long *>(sb + o_ctr);
    q.rowinfo = sb + o_rowinfo;
    q.bstat = sb + o_bstat;
    q.bits = reinterpret_cast<uint32_t *>(sb + o_bits);
    q.ex = reinterpret_cast<int32_t *>(sb + o_ex);
    q.en = reinterpret_cast<int32_t *>(sb + o_en);
    q.ek = reinterpret_cast<int32_t *>(sb + o_ek);
    q.list = reinterpret_cast<long long *>(sb + o_list);
    q.tbase = reinterpret_cast<unsigned long long *>(sb + o_tbase);
    SDNR_HIP(hipMemsetAsync(sb, 0, o_ex, ctx->stream));
    if (nent) SDNR_HIP(hipMemsetAsync(sb + o_ex, 0xFF, o_en - o_ex, ctx->stream));

    const size_t lds = (size_t)V * kFrrBytesPerV;
    sdnr_allow_lds(reinterpret_cast<const void *>(frr_base_kernel), lds);
    sdnr_allow_lds(reinterpret_cast<const void *>(frr_items_kernel), lds);
    int per_cu = (int)(SDNR_LDS_PER_CU / (lds ? lds : 1));
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);         // 2048 threads per CU
    const int64_t wide = (int64_t)ctx->num_cus * per_cu;

    if (nent) {
        const int64_t g = nscen < wide ? nscen : wide;
        hipLaunchKernelGGL(frr_entries_kernel, dim3((unsigned)g), dim3(256), 0, ctx->stream, V, E,
                           nscen, ctx->row_ptr, ctx->col, d_scen_off, scen_lo, scen_hi,
                           d_scen_edges, q, ctx->d_err);
    }
    {
        const int64_t g = nrows < wide ? nrows : wide;
        hipLaunchKernelGGL(frr_base_kernel, dim3((unsigned)g), dim3(kFrrThreads), lds, ctx->stream,
                           V, nrows, max_rounds, ctx->row_ptr, ctx->col, d_dst, d_nh, d_pair_off,
                           pair_lo, pair_hi, d_srcs, d_weight, q, ctx->d_err);
    }
    if (nent) {
        int64_t gy = (nent + 4095) / 4096;
        gy = gy > 64 ? 64 : gy;
        const int64_t gx = nrows < 4096 ? nrows : 4096;
        hipLaunchKernelGGL(frr_affected_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0,
                           ctx->stream, V, nrows, nent, d_dst, d_nh, q);
    }
    {
        int64_t most = (int64_t)E > npairs ? (int64_t)E : npairs;
        int64_t gx = (most + 1023) / 1024;
        gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
        const int64_t gy = nscen < 1024 ? nscen : 1024;
        hipLaunchKernelGGL(frr_spread_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0,
                           ctx->stream, E, nscen, npairs, q,
                           reinterpret_cast<unsigned long long *>(d_load),
                           reinterpret_cast<unsigned long long *>(d_stat), d_status);
    }
    int64_t g = wide < nitems ? wide : nitems;
    ctx->last_launches = 1;
    ctx->last_kernel = "frr_items_kernel<lds>";
    ctx->last_grid = g;
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    if (nent)
        hipLaunchKernelGGL(frr_items_kernel, dim3((unsigned)g), dim3(kFrrThreads), lds, ctx->stream,
                           V, E, nrows, max_rounds, ctx->row_ptr, ctx->col, d_dst, d_nh, d_backup,
                           d_pair_off, pair_lo, d_srcs, d_weight, d_scen_off, scen_lo, q,
                           reinterpret_cast<unsigned long long *>(d_load),
                           reinterpret_cast<unsigned long long *>(d_stat), d_status, npairs,
                           ctx->d_err);
    SDNR_HIP(hipGetLastError());
    if (ctx->timed) SDNR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    SDNR_HIP(hipMemcpyAsync(ctx->h_frr_items, q.ctr, sizeof(int64_t), hipMemcpyDeviceToHost,
                            ctx->stream));
    ctx->frr_items_pending = true;
    return SDNR_OK;
}

int sdnr_launch_frr_peak(sdnr_ctx *ctx, int32_t nscen, const uint64_t *d_load, uint64_t *d_peak,
                         int32_t *d_peak_edge)
{
    const int64_t g = nscen < 65535 ? nscen : 65535;
    hipLaunchKernelGGL(frr_peak_kernel, dim3((unsigned)g), dim3(kPeakThreads), 0, ctx->stream,
                       ctx->E, nscen, reinterpret_cast<const unsigned long long *>(d_load),
                       reinterpret_cast<unsigned long long *>(d_peak), d_peak_edge);
    SDNR_HIP(hipGetLastError());
    return SDNR_OK;
}
