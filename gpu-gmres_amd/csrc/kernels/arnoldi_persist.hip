// arnoldi_persist.hip -- one inner iteration's orthogonalization in one launch: k_arnoldi_persist, the
// two-scenario k_arnoldi_persist2, k_arnoldi_wide for long vectors.
#include "arnoldi.h"
#include "host.h"

namespace gg {

namespace {

// ---- persistent Arnoldi orthogonalization: <w,v_0>, the i+1 MGS steps, the
// norm, Givens and v_{i+1} = w/||w|| of inner iteration i in ONE launch.
// Block g owns the same units as in the per-step kernels (u = g*256 + t +
// j*G*256) and keeps them of w and of the current basis vector in registers
// across the steps, so a step reads one basis vector from HBM instead of
// w, v_k, v_{k+1} and writing w.  The per-step global sum is an all-gather of
// the G block partials through 8-byte granules (sentinel = not ready, relaxed
// agent-scope stores and polls, one row of G per step, re-armed per cycle);
// every block sums them in sum_partials' fixed order, so h is bit-identical to
// the per-step kernels'.  Needs all G blocks resident (checked on the host);
// every spin is bounded (err bit 0).
// Co-residency: the grid is sized from the occupancy API, which
// has over-promised on this pool (profiles/r03/r03_gather_ab.txt).  So the kernels
// do not trust it: the FIRST all-gather of a launch waits at most kResidSpin
// polls; a block that times out there sets DONE_ABORT in the control block
// (agent-scope atomic, drained before the block exits) and leaves.  A block
// entering the kernel returns at once when DONE_ABORT is set -- a block that
// was not resident can only be dispatched after some block exited, and only
// an aborting block exits early -- and every later poll that has to retry
// checks the flag every 256 retries, so the grid drains either way.
// DONE_ABORT gates the rest of the enqueued cycle off; the host restores the
// control block and reruns the cycle on the per-step kernels (same bits).

// the whole block: was the cycle aborted?  (entry check, one sc1 load)
__device__ __forceinline__ bool block_aborted(const DevState *ds)
{
    __shared__ int ab;
    if (threadIdx.x == 0) ab = ld_agent_i(&ds->done) & DONE_ABORT;
    __syncthreads();
    return ab != 0;
}
__device__ __forceinline__ void set_abort(DevState *ds)
{
    atomicOr(&ds->done, DONE_ABORT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // performed before this block exits
}

__device__ __forceinline__ unsigned long long poll_granule(const unsigned long long *p, int *err,
                                                          const int *abortw = nullptr)
{
    unsigned long long a = ld_agent(p);
    int spins = 0;
    while (a == kSentinel) {
        __builtin_amdgcn_s_sleep(1);
        a = ld_agent(p);
        if (abortw && (spins & 255) == 255 && (ld_agent_i(abortw) & DONE_ABORT)) break;
        if (++spins > kSpinLimit) {
            atomicOr(err, 1);
            break;
        }
    }
    return a;
}

// A thread's granules of a G-partial row (q = threadIdx.x + r*kBlock, G <=
// 1024): all of them loaded at once, then only the pending ones polled again --
// one memory round trip for the row instead of one per granule (a poll loop
// per granule serializes them: G = 544 put three sc1 round trips on every
// all-gather).  The sum is taken afterwards in q order, as before: same bits.
// Measured and not kept (round 5, profiles/r05/stage_ab.txt): two poll rounds
// in flight (a second load of every pending granule half a round trip after
// the first, here and in the blocks' slot poll): MGS 59.7 -> 75 us -- the
// extra polls slow the hand-offs more than they shorten the detection.
constexpr int kGatherPer = 4;
template <int NP>
__device__ __forceinline__ bool gather_row(const unsigned long long *row, int G, unsigned long long (&a)[NP],
                                           int limit, const int *abortw)
{
#pragma unroll
    for (int r = 0; r < NP; r++) {
        const int q = threadIdx.x + r * kBlock;
        a[r] = q < G ? ld_agent(row + q) : 0ull;
    }
    int spins = 0;
    while (true) {
        bool pend = false;
#pragma unroll
        for (int r = 0; r < NP; r++) pend |= a[r] == kSentinel;
        if (!pend) return true;
        __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int r = 0; r < NP; r++)
            if (a[r] == kSentinel) a[r] = ld_agent(row + threadIdx.x + r * kBlock);
        if (abortw && (spins & 255) == 255 && (ld_agent_i(abortw) & DONE_ABORT)) return false;
        if (++spins > limit) return false;
    }
}
template <int NP>
__device__ __forceinline__ double gather_row_sum(const unsigned long long (&a)[NP], int G)
{
    double v = 0.0;
#pragma unroll
    for (int r = 0; r < NP; r++)
        if (threadIdx.x + r * kBlock < G) v += __longlong_as_double((long long)a[r]);
    return v;
}

// NP: granules per thread the row may have (G <= NP * kBlock); NP = 0: one
// poll loop per granule (k_arnoldi_wide, whose 256 VGPRs are taken by w and
// the stream: the parallel form spills there)
template <int NP = kGatherPer>
__device__ __forceinline__ double gather_sum(const unsigned long long *row, int G, int *err, int &par,
                                             const int *abortw = nullptr)
{
    if constexpr (NP == 0) {
        double v = 0.0;
        for (int q = threadIdx.x; q < G; q += kBlock)
            v += __longlong_as_double((long long)poll_granule(row + q, err, abortw));
        return block_sum_pp(v, par);
    } else {
        unsigned long long a[NP];
        if (!gather_row<NP>(row, G, a, kSpinLimit, abortw) && !(abortw && (ld_agent_i(abortw) & DONE_ABORT)))
            atomicOr(err, 1);
        return block_sum_pp(gather_row_sum<NP>(a, G), par);
    }
}

// The launch's first all-gather with the co-residency bound: false = this
// block timed out (DONE_ABORT set) and must return (block-uniform)
template <int NP = kGatherPer>
__device__ __forceinline__ bool gather_first(const unsigned long long *row, int G, DevState *ds, int &par,
                                             double &h)
{
    double v = 0.0;
    int miss = 0;
    if constexpr (NP == 0) {
        for (int q = threadIdx.x; q < G; q += kBlock) {
            unsigned long long a = ld_agent(row + q);
            int spins = 0;
            while (a == kSentinel && !miss) {
                __builtin_amdgcn_s_sleep(1);
                a = ld_agent(row + q);
                if (++spins > kResidSpin) miss = 1;
            }
            v += __longlong_as_double((long long)a);
        }
    } else {
        unsigned long long a[NP];
        miss = gather_row<NP>(row, G, a, kResidSpin, nullptr) ? 0 : 1;
        v = gather_row_sum<NP>(a, G);
    }
    if (__syncthreads_or(miss)) {
        if (threadIdx.x == 0) set_abort(ds);
        return false;
    }
    h = block_sum_pp(v, par);
    return true;
}

// The sum of step k's partials as every block needs it.  LEADER: block 0
// alone gathers the row (gather_sum: the same order, the same bits) and
// publishes the sum in one granule hg; the other blocks' thread 0 polls that
// granule and hands the value over through LDS -- G line requests per poll
// round instead of G x G/32 on the few channels that hold the row, for one
// more hop.  Measured (C2 / C4, profiles/r03/r03_gather_ab.txt): k_arnoldi_wide
// (C4, streaming the basis beside the polls) 472.5 -> 456.6 us, so it leads;
// k_arnoldi_persist (C2) 73.2 -> 77.5 us, so every block gathers there.
template <bool LEADER, int NP = kGatherPer>
__device__ __forceinline__ double gather_h(const unsigned long long *row, unsigned long long *hg, int k, int G,
                                           int *err, int &par, const int *abortw)
{
    if (!LEADER || blockIdx.x == 0) {
        const double h = gather_sum<LEADER ? 0 : NP>(row, G, err, par, abortw);
        if (LEADER && threadIdx.x == 0) st_agent(hg, (unsigned long long)__double_as_longlong(h));
        return h;
    }
    __shared__ double hb[2];                    // alternating: steps k and k+2 are a block_sum apart
    if (threadIdx.x == 0) hb[k & 1] = __longlong_as_double((long long)poll_granule(hg, err, abortw));
    __syncthreads();
    return hb[k & 1];
}
// step 0 of a launch: gather_h with the co-residency bound on every wait
// (LEADER: block 0 gathers with the bound, the others' poll of its sum granule
// is bounded alike -- whichever block is missing, every waiting block times out)
template <bool LEADER, int NP = kGatherPer>
__device__ __forceinline__ bool gather_h_first(const unsigned long long *row, unsigned long long *hg, int G,
                                               DevState *ds, int &par, double &h)
{
    if (!LEADER || blockIdx.x == 0) {
        if (!gather_first<LEADER ? 0 : NP>(row, G, ds, par, h)) return false;
        if (LEADER && threadIdx.x == 0) st_agent(hg, (unsigned long long)__double_as_longlong(h));
        return true;
    }
    __shared__ double hb0;
    int miss = 0;
    if (threadIdx.x == 0) {
        unsigned long long a = ld_agent(hg);
        int spins = 0;
        while (a == kSentinel && !miss) {
            __builtin_amdgcn_s_sleep(1);
            a = ld_agent(hg);
            if (++spins > kResidSpin) miss = 1;
        }
        hb0 = __longlong_as_double((long long)a);
    }
    if (__syncthreads_or(miss)) {
        if (threadIdx.x == 0) set_abort(ds);
        return false;
    }
    h = hb0;
    return true;
}

// XCD-local form (GG_MGS_GATHER=2): ONE block per XCD (the first to arrive,
// elected per launch) gathers the step's G partials -- gather_sum, the same
// order, the same bits -- and stores the sum with a PLAIN store into its
// XCD's slot; the XCD's other blocks poll that slot (thread 0, sc1 loads).
// A plain store keeps the line in the XCD's L2, where the sc1 (L1-bypassing)
// polls of the same XCD find it: 234 / 677 ns a hop idle / streaming against
// 470 / 740 for sc1 stores (profiles/r04/r04_xcd_handoff.txt).  Correct by
// construction, not by placement: a block polls only the slot of the XCD it
// runs on (HW_REG_XCC_ID), which only a reducer ON that XCD writes.  8 pollers
// of the G-granule row instead of G.
constexpr int kXcdSlot = 16;                 // words per XCD slot (own 128-B line)
// (kXcds, xcc_id(), st_plain(): device.h)
// this block's role for the launch: the first block of its XCD to raise the
// XCD's election word to `seq` (strictly increasing per launch) reduces
__device__ __forceinline__ void xcd_elect(unsigned long long *elect, unsigned long long seq, bool &red,
                                          unsigned &xcc)
{
    __shared__ unsigned sx;
    __shared__ int sr;
    if (threadIdx.x == 0) {
        const unsigned x = xcc_id();
        sx = x;
        sr = atomicMax(elect + x * kXcdSlot, seq) < seq;
    }
    __syncthreads();
    red = sr != 0;
    xcc = sx;
}
// XG 3: a unit-holding block reduces for its XCD only when no reducer-only
// block has claimed the XCD for this launch (word 1 of the XCD's election
// slot).  The reducer-only blocks are blocks 0..kXcds-1, dispatched first and
// (round-robin) one per XCD, so the claim is normally there already; a short
// bounded wait covers its landing, and an XCD left without one (placement is
// not guaranteed) elects a unit-holding block as in XG 2.  Two reducers on one
// XCD store the same bits into its slot: harmless.
__device__ __forceinline__ void xcd_elect3(unsigned long long *elect, unsigned long long seq, bool &red,
                                           unsigned &xcc)
{
    __shared__ unsigned sx;
    __shared__ int sr;
    if (threadIdx.x == 0) {
        const unsigned x = xcc_id();
        sx = x;
        bool claimed = false;
        for (int t = 0; t < 16 && !claimed; t++) {
            claimed = ld_agent(elect + x * kXcdSlot + 1) == seq;
            if (!claimed) __builtin_amdgcn_s_sleep(8);
        }
        sr = !claimed && atomicMax(elect + x * kXcdSlot, seq) < seq;
    }
    __syncthreads();
    red = sr != 0;
    xcc = sx;
}
// step k's sum: slot = this XCD's word of step k
template <int NP>
__device__ __forceinline__ double gather_xcd(const unsigned long long *row, unsigned long long *slot, int k, int G,
                                            bool red, int *err, int &par, const int *abortw)
{
    if (red) {
        const double h = gather_sum<NP>(row, G, err, par, abortw);
        if (threadIdx.x == 0) st_plain(slot, (unsigned long long)__double_as_longlong(h));
        return h;
    }
    __shared__ double hb[2];                    // alternating: steps k and k+2 are a barrier apart
    if (threadIdx.x == 0) hb[k & 1] = __longlong_as_double((long long)poll_granule(slot, err, abortw));
    __syncthreads();
    return hb[k & 1];
}
template <int NP>
__device__ __forceinline__ bool gather_xcd_first(const unsigned long long *row, unsigned long long *slot, int G,
                                                 bool red, DevState *ds, int &par, double &h)
{
    if (red) {
        if (!gather_first<NP>(row, G, ds, par, h)) return false;
        if (threadIdx.x == 0) st_plain(slot, (unsigned long long)__double_as_longlong(h));
        return true;
    }
    __shared__ double hb0;
    int miss = 0;
    if (threadIdx.x == 0) {
        unsigned long long a = ld_agent(slot);
        int spins = 0;
        while (a == kSentinel && !miss) {
            __builtin_amdgcn_s_sleep(1);
            a = ld_agent(slot);
            if (++spins > kResidSpin) miss = 1;
        }
        hb0 = __longlong_as_double((long long)a);
    }
    if (__syncthreads_or(miss)) {
        if (threadIdx.x == 0) set_abort(ds);
        return false;
    }
    h = hb0;
    return true;
}

// XG: the all-gather's form -- 0 every block gathers, 2 XCD-local reducers
// (gather_xcd; xb = per step kXcds slots of kXcdSlot words, elect / seq the
// per-launch election)
// PF: v_{k+1} streamed while step k's sum is gathered (1), or after it (0):
// polls issued behind a wave's own in-flight basis loads wait for them (the
// memory returns in order) and the gather then also pays the stream's latency
constexpr int persist_np(int J) { return J >= 8 ? 0 : kGatherPer; }
template <int J, int XG, int PF>
__global__ __launch_bounds__(kBlock) void k_arnoldi_persist(Gate g, int i, int m, DevState *ds,
                                                            const double *__restrict__ w_in,
                                                            double *__restrict__ V, long long ldv,
                                                            double *H, double *cs, double *sn,
                                                            double *s, double *hist,
                                                            unsigned long long *gran, unsigned long long *hg,
                                                            long long units, int *err, unsigned long long *xb,
                                                            unsigned long long *elect, unsigned long long seq,
                                                            UnitMap um, long long *trace, const double *msc,
                                                            double *mout, unsigned long long *fill, long long nfill)
{
    // msc / mout (the split engine): also mout = v_{i+1} * msc, k_mul's product
    // for the next iteration's Mr (one pass fewer per iteration); fill: slots
    // < nfill set to the sentinel (the next flow U solve's x, its fill launch)
    // granules per thread loaded at once in the all-gathers (persist_np; J =
    // 8 polls them one by one: the parallel form would cost it an occupancy step)
    constexpr int kNP = persist_np(J);
    const long long t_in = trace ? (long long)__builtin_amdgcn_s_memrealtime() : 0;
    if (gated(g)) return;
    if (block_aborted(ds)) return;                            // co-residency (gather_first)
    // XG 3: the first kXcds blocks hold no units; they only reduce (below)
    constexpr int XR = XG == 3 ? kXcds : 0;
    const int G = gridDim.x - XR;                             // the blocks holding units
    const int ub = (int)blockIdx.x - XR;                      // this block's unit-block index
    const int *abortw = &ds->done;
    bool red = true;
    unsigned xcc = 0;
    auto xslot = [&](int k) { return xb + ((long long)k * kXcds + xcc) * kXcdSlot; };
    if constexpr (XG == 3) {
        if (ub < 0) {
            // reducer-only block: claim this XCD for the launch, then gather
            // every step's row (no basis loads in front of its polls) and
            // store the sum into the XCD's slot -- gather_xcd's reducer half
            int par = 0;
            __shared__ unsigned sxr;
            if (threadIdx.x == 0) {
                sxr = xcc_id();
                atomicMax(elect + sxr * kXcdSlot + 1, seq);
            }
            __syncthreads();
            xcc = sxr;
            double h;
            if (!gather_first<kNP>(gran, G, ds, par, h)) return;
            if (threadIdx.x == 0) st_plain(xslot(0), (unsigned long long)__double_as_longlong(h));
            for (int k = 1; k <= i + 1; k++) {
                h = gather_sum<kNP>(gran + (long long)k * G, G, err, par, abortw);
                if (threadIdx.x == 0) st_plain(xslot(k), (unsigned long long)__double_as_longlong(h));
            }
            return;
        }
        xcd_elect3(elect, seq, red, xcc);
    }
    if constexpr (XG == 2) xcd_elect(elect, seq, red, xcc);
    const long long stride = (long long)G * kBlock;
    const long long u0 = ub * (long long)kBlock + threadIdx.x;
    // diagnostics (GG_MGS_TRACE): per step the start, h known, partial formed,
    // partial published -- row 0 unit-block 0, row 1 the reducer of XCD 0
    const int trow = !trace ? -1 : ub == 0 ? 0 : (red && xcc == 0 && XG == 2) ? 1 : -1;
    auto stamp = [&](int k, int ph) {
        if (trow >= 0 && threadIdx.x == 0)
            trace[((long long)trow * (i + 2) + k) * 4 + ph] = (long long)__builtin_amdgcn_s_memrealtime();
    };
    // the launch's head and tail (row 2): 0 entry, 1 gate / abort / election
    // resolved, 2 w and v_0 landed, 4 the Givens block done, 5 v_{i+1} stored
    auto stamp_ht = [&](int ph, long long t = -1) {
        if (trow == 0 && threadIdx.x == 0)
            trace[(long long)2 * (i + 2) * 4 + ph] = t >= 0 ? t : (long long)__builtin_amdgcn_s_memrealtime();
    };
    stamp_ht(0, t_in);
    stamp_ht(1);
    double2 w[J], vk[J], vn[J];
    [[maybe_unused]] double2 vl[PF == 2 ? J : 1];             // PF 2: the third basis buffer
    bool val[J];                                              // unit holds a real row (UnitMap)
#pragma unroll
    for (int j = 0; j < J; j++) {
        const long long u = u0 + j * stride;
        val[j] = u < units && unit_real(um, u);
        if (val[j]) {
            w[j] = ld2(w_in, u);
            vk[j] = ld2(V, u);
        }
    }
    auto load_v = [&](int q, double2 *dst) {                  // basis vector q, streamed
        const double *vp = V + (long long)q * ldv;
#pragma unroll
        for (int j = 0; j < J; j++)
            if (val[j]) dst[j] = ld2_nt(vp, u0 + j * stride);
    };
    if constexpr (PF == 2) {
        if (i >= 1) load_v(1, vn);                            // v_1, behind w and v_0
    }
    // unit-block 0 keeps the column's first kRotLds stored rotations cs / sn in
    // LDS (1 KB: a restart of up to 65 lies in it whole; the entries beyond it
    // are read from memory where they are used, in a gather's shadow).  One
    // coalesced, looped pass, in program order BEHIND the loads of w and v_0 so
    // that its wait delays none of them; visible after publish(0)'s barrier.
    constexpr int kRotLds = 64;
    __shared__ double rot_c[kRotLds], rot_s[kRotLds];
    if (ub == 0) {
        const int nrot = i < kRotLds ? i : kRotLds;
        for (int k = threadIdx.x; k < nrot; k += kBlock) {
            rot_c[k] = cs[k];
            rot_s[k] = sn[k];
        }
    }
    int par = 0;                                              // block_sum_pp's LDS row
    auto publish = [&](int k, double acc) {
        acc = block_sum_pp(acc, par);
        if (threadIdx.x == 0) st_agent(gran + (long long)k * G + ub, (unsigned long long)__double_as_longlong(acc));
    };
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < J; j++)
        if (val[j]) {
            acc += w[j].x * vk[j].x;
            acc += w[j].y * vk[j].y;
        }
    stamp_ht(2);
    publish(0, acc);                                          // <w, v_0>
    double *const Hc = H + i * (m + 1);                       // column i (unit-block 0's thread 0)
    double hlo = 0.0;                                         // its entry still to be rotated
    // step k: h_k, w -= h_k v_k, the partial of the next dot (v_{k+1}, or the
    // norm), published.  cur = v_k, nxt = v_{k+1} (loaded), lnd = the buffer
    // v_{k+2} lands in (PF 2; the three rotate, no register copies -- a copy of
    // a landing buffer would wait for its loads)
    auto step = [&](int k, double2 *cur, double2 *nxt, double2 *lnd) -> bool {
        stamp(k, 0);
        if constexpr (PF == 1) {
            if (k < i) load_v(k + 1, nxt);                    // v_{k+1}, in flight during the sum
        }
        double h;
        if (k == 0) {
            if (XG >= 2 ? !gather_xcd_first<kNP>(gran, xslot(0), G, red, ds, par, h)
                        : !gather_h_first<false, kNP>(gran, hg, G, ds, par, h))
                return false;
        } else if constexpr (XG >= 2) {
            h = gather_xcd<kNP>(gran + (long long)k * G, xslot(k), k, G, red, err, par, abortw);
        } else {
            h = gather_h<false, kNP>(gran + (long long)k * G, hg + k, k, G, err, par, abortw);
        }
        if constexpr (PF == 0) {
            __builtin_amdgcn_sched_barrier(0);
            if (k < i) load_v(k + 1, nxt);                    // v_{k+1} after the sum
        }
        if constexpr (PF == 2) {
            // v_{k+2} issued after this step's polls, which so find no basis
            // loads of their own in front of them (v_{k+1} went out a step ago)
            __builtin_amdgcn_sched_barrier(0);
            if (k + 2 <= i) load_v(k + 2, lnd);
        }
        stamp(k, 1);
        const double a = -h;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < J; j++) {
            if (val[j]) {
                w[j].x = a * cur[j].x + w[j].x;
                w[j].y = a * cur[j].y + w[j].y;
                const double2 o = (k < i) ? nxt[j] : w[j];    // next dot: v_{k+1}, or the norm
                acc += w[j].x * o.x;
                acc += w[j].y * o.y;
            }
        }
        stamp(k, 2);
        publish(k + 1, acc);
        stamp(k, 3);
        // the column, rotated as its entries arrive (givens_absorb): h_k lets
        // rotation k-1 go and makes Hc[k-1] final -- behind the publication,
        // in the next gather's shadow
        if (ub == 0 && threadIdx.x == 0) {
            if (k == 0) {
                hlo = h;
            } else {
                const int q = k - 1;
                const double c = q < kRotLds ? rot_c[q] : cs[q], r = q < kRotLds ? rot_s[q] : sn[q];
                Hc[q] = givens_absorb(hlo, h, c, r);
            }
        }
        return true;
    };
    if constexpr (PF == 2) {
        for (int k = 0; k <= i; k += 3) {
            if (!step(k, vk, vn, vl)) return;
            if (k + 1 > i) break;
            step(k + 1, vn, vl, vk);
            if (k + 2 > i) break;
            step(k + 2, vl, vk, vn);
        }
    } else {
        for (int k = 0; k <= i; k += 2) {
            if (!step(k, vk, vn, nullptr)) return;
            if (k + 1 > i) break;
            step(k + 1, vn, vk, nullptr);
        }
    }
    stamp(i + 1, 0);
    // what the column's last step reads (s[i], s[i+1], normb, tol, hist_len):
    // requested here, in flight during the norm's gather
    GivensIn gin = {};
    if (ub == 0 && threadIdx.x == 0) gin = givens_load(s, ds, i);
    const double hn = sqrt(XG >= 2 ? gather_xcd<kNP>(gran + (long long)(i + 1) * G, xslot(i + 1), i + 1, G, red, err, par,
                                                abortw)
                                   : gather_h<false, kNP>(gran + (long long)(i + 1) * G, hg + i + 1, i + 1, G, err, par,
                                                     abortw));
    stamp(i + 1, 1);
    if (ub == 0 && threadIdx.x == 0) {                       // rotations 0..i-1 are applied: registers, then stores
        givens_finish(hlo, hn, gin, i, Hc, cs, sn, s, hist, ds);
        stamp_ht(4);
    }
    const double inv = (hn != 0.0) ? 1.0 / hn : 0.0;
    double *vout = V + (long long)(i + 1) * ldv;
#pragma unroll
    for (int j = 0; j < J; j++) {
        const long long u = u0 + j * stride;
        if (val[j]) {
            double2 a = w[j];
            a.x = inv * a.x;
            a.y = inv * a.y;
            st2(vout, u, a);
            if (mout) {
                const double2 c = ld2(msc, u);
                st2(mout, u, make_double2(a.x * c.x, a.y * c.y));
            }
        } else if (mout && u < units) {
            // padding: k_mul's product of the slot as it stands (never written here)
            const double2 a = ld2(vout, u), c = ld2(msc, u);
            st2(mout, u, make_double2(a.x * c.x, a.y * c.y));
        }
        if (fill && u < units) {
            if (2 * u < nfill) fill[2 * u] = kSentinel;
            if (2 * u + 1 < nfill) fill[2 * u + 1] = kSentinel;
        }
    }
    if (trow == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (diagnostics only) the stores performed
        stamp_ht(5);
    }
}

// ---- two scenarios per launch (the many-RHS batch, batch.hip) ----------------
// k_arnoldi_persist's default form (XCD-local reducers, v_{k+1} streamed during
// the gather) for two scenarios at once: scenario q's buffers q * zs bytes after
// scenario 0's; per step the two rows are gathered together -- every granule of
// both loaded at once, the pending ones re-polled, then each row summed in the
// same q order (gather_row_sum + block_sum_pp: the same bits) -- so the two
// scenarios share the step's hand-off latency instead of paying it in two
// launches.  A gated scenario (converged) is skipped inside the launch.
template <int J>
__device__ __forceinline__ void gather2_xcd(const unsigned long long *row0, const unsigned long long *row1,
                                            unsigned long long *slot0, unsigned long long *slot1, int G, bool red,
                                            const bool (&act)[2], int *err, int &par, int limit,
                                            const int *abort0, const int *abort1, double (&h)[2], int &miss)
{
    constexpr int NP = kGatherPer;
    __shared__ double hb2[2][2];
    if (red) {
        unsigned long long a[2][NP];
        const unsigned long long *rows[2] = {row0, row1};
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int r = 0; r < NP; r++) {
                const int k = threadIdx.x + r * kBlock;
                a[q][r] = (act[q] && k < G) ? ld_agent(rows[q] + k) : 0ull;
            }
        int spins = 0;
        while (true) {
            bool pend = false;
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int r = 0; r < NP; r++) pend |= a[q][r] == kSentinel;
            if (!pend) break;
            __builtin_amdgcn_s_sleep(1);
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int r = 0; r < NP; r++)
                    if (a[q][r] == kSentinel) a[q][r] = ld_agent(rows[q] + threadIdx.x + r * kBlock);
            if ((spins & 255) == 255 && ((act[0] && (ld_agent_i(abort0) & DONE_ABORT)) ||
                                         (act[1] && (ld_agent_i(abort1) & DONE_ABORT)))) {
                miss = 1;
                break;
            }
            if (++spins > limit) {
                miss = 1;
                break;
            }
        }
        unsigned long long *slots[2] = {slot0, slot1};
#pragma unroll
        for (int q = 0; q < 2; q++) {
            if (!act[q]) continue;                                    // (block-uniform)
            h[q] = block_sum_pp(gather_row_sum<NP>(a[q], G), par);
            if (threadIdx.x == 0) st_plain(slots[q], (unsigned long long)__double_as_longlong(h[q]));
        }
        return;
    }
    // the XCD's other blocks: thread q polls scenario q's slot
    if (threadIdx.x < 2 && act[threadIdx.x]) {
        const unsigned long long *sl = threadIdx.x ? slot1 : slot0;
        unsigned long long v = ld_agent(sl);
        int spins = 0;
        while (v == kSentinel) {
            __builtin_amdgcn_s_sleep(1);
            v = ld_agent(sl);
            const int *ab = threadIdx.x ? abort1 : abort0;
            if ((spins & 255) == 255 && (ld_agent_i(ab) & DONE_ABORT)) {
                miss = 1;
                break;
            }
            if (++spins > limit) {
                miss = 1;
                break;
            }
        }
        hb2[par & 1][threadIdx.x] = __longlong_as_double((long long)v);
    }
    __syncthreads();
    h[0] = hb2[par & 1][0];
    h[1] = hb2[par & 1][1];
    par ^= 1;
}

// three blocks per CU (168 VGPRs at J = 4, 22 spilled): C5's grid of 532
// blocks co-resident (2 per CU at 192 VGPRs would hold 512) -- C5 with 8
// scenarios 10,606 -> 11,255 it/s, MGS 54.3 -> 45.5 us per pair of scenarios
// (profiles/r06/r06x_c5_pair.txt)
template <int J>
__global__ __launch_bounds__(kBlock, 3) void k_arnoldi_persist2(Gate g, long long zs, int i, int m, DevState *ds,
                                                             const double *__restrict__ w_in,
                                                             double *__restrict__ V, long long ldv, double *H,
                                                             double *cs, double *sn, double *s, double *hist,
                                                             unsigned long long *gran, long long units, int *err,
                                                             unsigned long long *xb, unsigned long long *elect,
                                                             unsigned long long seq, UnitMap um)
{
    bool act[2];
    DevState *dsq[2] = {ds, zp(ds, zs, 1)};
    __shared__ int sab[2];
    if (threadIdx.x < 2) sab[threadIdx.x] = ld_agent_i(&dsq[threadIdx.x]->done) & DONE_ABORT;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; q++) act[q] = !gated_z(g, zs, q) && !sab[q];
    if (!act[0] && !act[1]) return;
    const int G = gridDim.x;
    const int ub = (int)blockIdx.x;
    bool red = true;
    unsigned xcc = 0;
    xcd_elect(elect, seq, red, xcc);
    const long long stride = (long long)G * kBlock;
    const long long u0 = ub * (long long)kBlock + threadIdx.x;
    const double *wq[2] = {w_in, zp(w_in, zs, 1)};
    double *Vq[2] = {V, zp(V, zs, 1)};
    unsigned long long *gq[2] = {gran, zp(gran, zs, 1)};
    unsigned long long *xq[2] = {xb, zp(xb, zs, 1)};
    const int *abw[2] = {&dsq[0]->done, &dsq[1]->done};
    auto xslot = [&](int q, int k) { return xq[q] + ((long long)k * kXcds + xcc) * kXcdSlot; };
    double2 w[2][J], vk[2][J], vn[2][J];
    bool val[J];
#pragma unroll
    for (int j = 0; j < J; j++) {
        const long long u = u0 + j * stride;
        val[j] = u < units && unit_real(um, u);
#pragma unroll
        for (int q = 0; q < 2; q++)
            if (val[j] && act[q]) {
                w[q][j] = ld2(wq[q], u);
                vk[q][j] = ld2(Vq[q], u);
            }
    }
    int par = 0;
    // both scenarios' partials of one step, each with block_sum_pp's tree
    auto publish = [&](int k, double (&acc)[2]) {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            if (!act[q]) continue;
            const double a = block_sum_pp(acc[q], par);
            if (threadIdx.x == 0) st_agent(gq[q] + (long long)k * G + ub, (unsigned long long)__double_as_longlong(a));
        }
    };
    {
        double acc[2] = {0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int j = 0; j < J; j++)
                if (val[j] && act[q]) {
                    acc[q] += w[q][j].x * vk[q][j].x;
                    acc[q] += w[q][j].y * vk[q][j].y;
                }
        publish(0, acc);                                          // <w, v_0>
    }
    auto step = [&](int k, double2 (&cur)[2][J], double2 (&nxt)[2][J]) -> bool {
        if (k < i) {                                              // v_{k+1}, in flight during the gather
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (!act[q]) continue;
                const double *vp = Vq[q] + (long long)(k + 1) * ldv;
#pragma unroll
                for (int j = 0; j < J; j++)
                    if (val[j]) nxt[q][j] = ld2_nt(vp, u0 + j * stride);
            }
        }
        double h[2] = {0.0, 0.0};
        int miss = 0;
        gather2_xcd<J>(gq[0] + (long long)k * G, gq[1] + (long long)k * G, xslot(0, k), xslot(1, k), G, red, act,
                       err, par, k == 0 ? kResidSpin : kSpinLimit, abw[0], abw[1], h, miss);
        if (k == 0) {
            // the launch's first all-gather bounds the co-residency wait
            if (__syncthreads_or(miss)) {
                if (threadIdx.x < 2 && act[threadIdx.x]) set_abort(dsq[threadIdx.x]);
                return false;
            }
        } else if (miss && !(ld_agent_i(abw[0]) & DONE_ABORT) && !(ld_agent_i(abw[1]) & DONE_ABORT)) {
            atomicOr(err, 1);                                     // a wait timed out
        }
        double acc[2] = {0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 2; q++) {
            if (!act[q]) continue;
            if (ub == 0 && threadIdx.x == 0) zp(H, zs, q)[k + i * (m + 1)] = h[q];
            const double a = -h[q];
#pragma unroll
            for (int j = 0; j < J; j++) {
                if (val[j]) {
                    w[q][j].x = a * cur[q][j].x + w[q][j].x;
                    w[q][j].y = a * cur[q][j].y + w[q][j].y;
                    const double2 o = (k < i) ? nxt[q][j] : w[q][j];
                    acc[q] += w[q][j].x * o.x;
                    acc[q] += w[q][j].y * o.y;
                }
            }
        }
        publish(k + 1, acc);
        return true;
    };
    for (int k = 0; k <= i; k += 2) {
        if (!step(k, vk, vn)) return;
        if (k + 1 > i) break;
        step(k + 1, vn, vk);
    }
    double hn[2] = {0.0, 0.0};
    {
        int miss = 0;
        gather2_xcd<J>(gq[0] + (long long)(i + 1) * G, gq[1] + (long long)(i + 1) * G, xslot(0, i + 1),
                       xslot(1, i + 1), G, red, act, err, par, kSpinLimit, abw[0], abw[1], hn, miss);
        if (miss && !(ld_agent_i(abw[0]) & DONE_ABORT) && !(ld_agent_i(abw[1]) & DONE_ABORT)) atomicOr(err, 1);
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
        if (!act[q]) continue;
        const double hq = sqrt(hn[q]);
        if (ub == 0 && threadIdx.x == 0)                          // the column from memory, batched loads
            givens_column(i, hq, zp(H, zs, q) + i * (m + 1), zp(cs, zs, q), zp(sn, zs, q), zp(s, zs, q),
                          zp(hist, zs, q), dsq[q]);
        const double inv = (hq != 0.0) ? 1.0 / hq : 0.0;
        double *vout = Vq[q] + (long long)(i + 1) * ldv;
#pragma unroll
        for (int j = 0; j < J; j++) {
            if (val[j]) {
                double2 a = w[q][j];
                a.x = inv * a.x;
                a.y = inv * a.y;
                st2(vout, u0 + j * stride, a);
            }
        }
    }
}

// k_arnoldi_wide -- the same inner iteration for vectors too long for
// k_arnoldi_persist's registers (C4: 11.6M slots): only w stays on chip (kWideJR
// units per thread in registers, kWideJL in LDS), v_k and v_{k+1} are streamed
// (non-temporal) at every step, kWideD units ahead of their use -- 16 B per
// slot and step against the per-step kernels' 32 (w read and written).  Same
// reduction tree as k_dot / k_mgs_step (G blocks of 256 threads, grid-stride
// units, per thread ascending j, block_sum, G partials summed in sum_partials
// order), so it is bit-identical to the per-step path.  Needs every block
// co-resident (host: kWideG blocks, two per CU).
// kWideJS of a thread's units of v_{k+1} are kept in LDS from step k, where they
// are streamed for the next dot, to step k+1, where they are v_k (and v_0 from
// the first dot to step 0): that share of the basis is read from HBM once per
// step instead of twice (LDS: 2 blocks x (kWideJL + kWideJS) x 256 x 16 B)
#ifndef GG_WIDE_STASH
#define GG_WIDE_STASH 14
#endif
constexpr int kWideJR = 40, kWideJL = 5, kWideD = 8, kWideJS = GG_WIDE_STASH;
#ifndef GG_WIDE_NEXT_NT
#define GG_WIDE_NEXT_NT 0
#endif
__global__ __launch_bounds__(kBlock, 2) void k_arnoldi_wide(Gate g, int i, int m, DevState *ds,
                                                            const double *__restrict__ w_in,
                                                            double *__restrict__ V, long long ldv,
                                                            double *H, double *cs, double *sn,
                                                            double *s, double *hist,
                                                            unsigned long long *gran, unsigned long long *hg,
                                                            long long units, int *err, UnitMap um)
{
    constexpr int J = kWideJR + kWideJL;
    if (gated(g)) return;
    if (block_aborted(ds)) return;                            // co-residency (gather_first)
    const int *abortw = &ds->done;
    __shared__ double2 wl[kWideJL * kBlock];
    __shared__ double2 vst[(kWideJS > 0 ? kWideJS : 1) * kBlock];   // v_{k+1} (then v_k) of units j < kWideJS
    const int G = gridDim.x;
    const int stride = G * kBlock;                      // units (vectors < 2^31 units: host check)
    const int u0 = blockIdx.x * kBlock + threadIdx.x;
    // this thread's units u0 + j stride, j < nval
    const int nval = units > u0 ? (int)((units - u0 + stride - 1) / stride) : 0;
    // (no padding skip here: the validity mask costs this kernel its registers
    // -- 148 VGPRs spilled -- at 256 VGPRs; um is unused)
    (void)um;
    auto ok = [&](int j) { return j < nval; };
    double2 wr[kWideJR];
    auto wget = [&](int j) -> double2 { return j < kWideJR ? wr[j] : wl[(j - kWideJR) * kBlock + threadIdx.x]; };
    auto wset = [&](int j, double2 v) {
        if (j < kWideJR) wr[j] = v;
        else wl[(j - kWideJR) * kBlock + threadIdx.x] = v;
    };
    int gpar = 0;                                       // block_sum_pp's LDS row
    auto publish = [&](int k, double acc) {
        acc = block_sum_pp(acc, gpar);
        if (threadIdx.x == 0) st_agent(gran + (long long)k * G + blockIdx.x, (unsigned long long)__double_as_longlong(acc));
    };
    // streaming ring: slot j % kWideD holds unit j's v_k (and v_{k+1}).  The
    // unit offsets are recomputed in every step from a laundered base (not
    // hoisted: 45 live offsets would not fit beside w)
    double2 pk[kWideD], pn[kWideD];
    // v_{k+1} is read again as v_k in the next step: GG_WIDE_NEXT_NT=0 reads it
    // with the default policy (it may stay in the Infinity Cache for that
    // second read), 1 streams it non-temporally like v_k's last read
    // stash: v_k's units j < kWideJS come from LDS (written one step earlier)
    auto fetch = [&](int j, int ub, const double2 *vkp, const double2 *vnp, bool stash) {
        if (j < J && ok(j)) {
            if (stash && j < kWideJS) {
                pk[j % kWideD] = vst[j * kBlock + threadIdx.x];
            } else {
                const dbl2v a = __builtin_nontemporal_load(reinterpret_cast<const dbl2v *>(vkp) + ub + j * stride);
                pk[j % kWideD] = make_double2(a.x, a.y);
            }
            if (vnp) {
                if constexpr (GG_WIDE_NEXT_NT) {
                    const dbl2v c = __builtin_nontemporal_load(reinterpret_cast<const dbl2v *>(vnp) + ub + j * stride);
                    pn[j % kWideD] = make_double2(c.x, c.y);
                } else {
                    pn[j % kWideD] = vnp[ub + j * stride];
                }
            }
        }
    };
    auto vec = [&](const double *p) { return reinterpret_cast<const double2 *>(p); };
    double acc = 0.0;
    {
        int ub = u0;
        asm volatile("" : "+v"(ub));
#pragma unroll
        for (int j = 0; j < kWideD; j++) fetch(j, ub, vec(V), nullptr, false);
#pragma unroll
        for (int j = 0; j < J; j++) {
            if (ok(j)) {
                const double2 wv = vec(w_in)[ub + j * stride];
                wset(j, wv);
                const double2 v0 = pk[j % kWideD];
                acc += wv.x * v0.x;
                acc += wv.y * v0.y;
                if (j < kWideJS) vst[j * kBlock + threadIdx.x] = v0;     // v_0 again at step 0
            }
            fetch(j + kWideD, ub, vec(V), nullptr, false);
        }
    }
    publish(0, acc);                                          // <w, v_0>
    for (int k = 0; k <= i; k++) {
        const double2 *vkp = vec(V + (long long)k * ldv);
        const double2 *vnp = (k < i) ? vec(V + (long long)(k + 1) * ldv) : nullptr;
        int ub = u0;
        asm volatile("" : "+v"(ub));
#pragma unroll
        for (int j = 0; j < kWideD; j++) fetch(j, ub, vkp, vnp, true);    // in flight during the sum
        double h;
        if (k == 0) {
            if (!gather_h_first<true>(gran, hg, G, ds, gpar, h)) return;
        } else {
            h = gather_h<true>(gran + (long long)k * G, hg + k, k, G, err, gpar, abortw);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) H[k + i * (m + 1)] = h;
        const double a = -h;
        acc = 0.0;
#pragma unroll
        for (int j = 0; j < J; j++) {
            if (ok(j)) {
                double2 wv = wget(j);
                const double2 vk = pk[j % kWideD];
                wv.x = a * vk.x + wv.x;
                wv.y = a * vk.y + wv.y;
                wset(j, wv);
                const double2 o = vnp ? pn[j % kWideD] : wv;    // next dot: v_{k+1}, or the norm
                acc += wv.x * o.x;
                acc += wv.y * o.y;
                if (vnp && j < kWideJS) vst[j * kBlock + threadIdx.x] = o;   // v_k of the next step
            }
            fetch(j + kWideD, ub, vkp, vnp, true);
        }
        publish(k + 1, acc);
    }
    const double hn = sqrt(gather_h<true>(gran + (long long)(i + 1) * G, hg + i + 1, i + 1, G, err, gpar, abortw));
    // (the column from memory, as the per-step kernels: an on-chip column would
    // cost this kernel registers it does not have)
    if (blockIdx.x == 0 && threadIdx.x == 0) givens_column(i, hn, H + i * (m + 1), cs, sn, s, hist, ds);
    const double inv = (hn != 0.0) ? 1.0 / hn : 0.0;
    double2 *vout = reinterpret_cast<double2 *>(V + (long long)(i + 1) * ldv);
#pragma unroll
    for (int j = 0; j < J; j++) {
        if (ok(j)) {
            double2 a = wget(j);
            a.x = inv * a.x;
            a.y = inv * a.y;
            vout[u0 + j * stride] = a;
        }
    }
}

}  // namespace

// ======================================================= host launchers
// tests: GG_PERSIST_TEST_LDS = dynamic LDS bytes added to the persistent
// orthogonalization launches, so that fewer blocks fit than the grid needs
// (the co-residency abort and the per-step rerun, gather_first)
static size_t persist_test_lds()
{
    const char *e = std::getenv("GG_PERSIST_TEST_LDS");
    return e ? (size_t)std::max(0, atoi(e)) : 0;
}

#ifndef GG_MGS_GATHER_DEFAULT
#define GG_MGS_GATHER_DEFAULT 2
#endif
constexpr int kMgsGatherDefault = GG_MGS_GATHER_DEFAULT;

int arnoldi_persist_units(int G, long long Ppad)
{
    const long long units = Ppad / 2, per = (long long)G * kBlock;
    const int J = (int)((units + per - 1) / per);
    return J <= 1 ? 1 : J <= 2 ? 2 : J <= 4 ? 4 : J <= 8 ? 8 : 0;
}

// the k_arnoldi_persist instantiation for J units per thread under the
// current GG_MGS_GATHER / GG_MGS_PREFETCH (one choice for the occupancy query
// and the launch: ADVICE r4)
using PersistFn = void (*)(Gate, int, int, DevState *, const double *, double *, long long, double *, double *,
                           double *, double *, double *, unsigned long long *, unsigned long long *, long long, int *,
                           unsigned long long *, unsigned long long *, unsigned long long, UnitMap, long long *,
                           const double *, double *, unsigned long long *, long long);
template <int XG, int PF>
PersistFn persist_fn_j(int J)
{
    if constexpr (PF == 2) {
        return J == 1 ? k_arnoldi_persist<1, XG, PF> : J == 2 ? k_arnoldi_persist<2, XG, PF>
                                                               : k_arnoldi_persist<4, XG, PF>;
    } else {
        return J == 1   ? k_arnoldi_persist<1, XG, PF>
               : J == 2 ? k_arnoldi_persist<2, XG, PF>
               : J == 4 ? k_arnoldi_persist<4, XG, PF>
                        : k_arnoldi_persist<8, XG, PF>;
    }
}
// GG_MGS_GATHER / GG_MGS_PREFETCH onto the instantiation <J, XG, PF> that runs:
// the one mapping behind the launch, the occupancy query, the reducer-only
// blocks (arnoldi_persist_extra) and the name gg_mgs_kernel reports
void persist_form(int J, int &xg, int &pf)
{
    const int g = mgs_gather_form(), p = mgs_prefetch();
    if (g == 2 && p == 2 && J <= 4) xg = 2, pf = 2;
    else if (g == 3 && p) xg = 3, pf = 1;
    else if (g >= 2) xg = 2, pf = p ? 1 : 0;
    else xg = 0, pf = p ? 1 : 0;
}
PersistFn persist_fn(int J)
{
    int xg, pf;
    persist_form(J, xg, pf);
    if (xg == 2 && pf == 2) return persist_fn_j<2, 2>(J);
    if (xg == 3) return persist_fn_j<3, 1>(J);
    if (xg == 2) return pf ? persist_fn_j<2, 1>(J) : persist_fn_j<2, 0>(J);
    return pf ? persist_fn_j<0, 1>(J) : persist_fn_j<0, 0>(J);
}
int arnoldi_persist_extra(int J)
{
    int xg, pf;
    persist_form(J, xg, pf);
    return xg == 3 ? kXcds : 0;       // <J, 3, 1>: one reducer-only block per XCD
}
std::string arnoldi_persist_name(int J)
{
    int xg, pf;
    persist_form(J, xg, pf);
    return "k_arnoldi_persist<" + std::to_string(J) + ", " + std::to_string(xg) + ", " + std::to_string(pf) + ">";
}

// blocks of the J-unit instantiation that can be resident at once
int arnoldi_persist_max_blocks(int J)
{
    if (J != 1 && J != 2 && J != 4 && J != 8) return 0;
    // the instantiation launch_arnoldi_persist launches
    return resident_blocks(persist_fn(J), kBlock);
}

// k_arnoldi_wide: usable when G = kWideG blocks of kWideJR + kWideJL units per
// thread cover the vectors and every block is co-resident
bool arnoldi_wide_ok(int G, long long Ppad)
{
    static int maxb = -1;
    if (maxb < 0) maxb = resident_blocks(k_arnoldi_wide, kBlock);
    const long long units = Ppad / 2;
    return G == kWideG && G <= maxb && units <= (long long)G * kBlock * (kWideJR + kWideJL) && units < (1LL << 31);
}

void launch_arnoldi_wide(Gate g, int i, int m, DevState *ds, const double *w, double *V, long long ldv,
                         double *H, double *cs, double *sn, double *s, double *hist,
                         unsigned long long *gran, unsigned long long *hg, int G, long long Ppad, int *err,
                         const UnitMap &um, hipStream_t st)
{
    k_arnoldi_wide<<<G, kBlock, persist_test_lds(), st>>>(g, i, m, ds, w, V, ldv, H, cs, sn, s, hist, gran, hg,
                                                          Ppad / 2, err, um);
}

#ifndef GG_MGS_PREFETCH_DEFAULT
#define GG_MGS_PREFETCH_DEFAULT 1
#endif
int mgs_prefetch()
{
    // 1: v_{k+1} streamed during step k's gather, 0: after it, 2: v_{k+2}
    // issued after step k's gather (prefetch distance 2, J <= 4)
    const char *e = std::getenv("GG_MGS_PREFETCH");
    return e ? std::min(std::max(atoi(e), 0), 2) : GG_MGS_PREFETCH_DEFAULT;
}
int mgs_gather_form()
{
    // 0: every block gathers, 2: XCD-local reducers elected among the blocks,
    // 3: XCD-local reducer-only blocks (kXcds extra blocks)
    const char *e = std::getenv("GG_MGS_GATHER");
    return e ? (atoi(e) == 2 ? 2 : atoi(e) == 3 ? 3 : 0) : kMgsGatherDefault;
}

void launch_arnoldi_persist(Gate g, int i, int m, DevState *ds, const double *w, double *V,
                            long long ldv, double *H, double *cs, double *sn, double *s,
                            double *hist, unsigned long long *gran, unsigned long long *hg, int G, long long Ppad,
                            int *err, unsigned long long *xb, unsigned long long *elect, unsigned long long seq,
                            const UnitMap &um, hipStream_t st, long long *trace, const double *msc, double *mout,
                            double *fill, long long nfill)
{
    const int J = arnoldi_persist_units(G, Ppad);
    GG_REQUIRE(persist_np(J) == 0 || G <= persist_np(J) * kBlock, GG_EINVAL,
               "k_arnoldi_persist: grid beyond the all-gather's reach");
    const PersistFn f = persist_fn(J);
    const int extra = arnoldi_persist_extra(J);                                 // reducer-only blocks
    f<<<G + extra, kBlock, persist_test_lds(), st>>>(g, i, m, ds, w, V, ldv, H, cs, sn, s, hist, gran, hg, Ppad / 2,
                                                     err, xb, elect, seq, um, trace, msc, mout,
                                                     reinterpret_cast<unsigned long long *>(fill), fill ? nfill : 0);
}

// the two-scenario persistent orthogonalization (k_arnoldi_persist2): 0 when
// the vectors take no J or the grid cannot be co-resident
int arnoldi_persist2_units(int G, long long Ppad)
{
    const int J = arnoldi_persist_units(G, Ppad);
    if (J != 1 && J != 2 && J != 4) return 0;
    static int cached[5] = {-1, -1, -1, -1, -1};
    if (cached[J] < 0)
        cached[J] = resident_blocks(J == 1 ? k_arnoldi_persist2<1> : J == 2 ? k_arnoldi_persist2<2> : k_arnoldi_persist2<4>,
                                    kBlock);
    return G <= cached[J] ? J : 0;
}
void launch_arnoldi_persist2(Gate g, long long zs, int i, int m, DevState *ds, const double *w, double *V,
                             long long ldv, double *H, double *cs, double *sn, double *s, double *hist,
                             unsigned long long *gran, int G, long long Ppad, int *err, unsigned long long *xb,
                             unsigned long long *elect, unsigned long long seq, const UnitMap &um, hipStream_t st)
{
    const int J = arnoldi_persist_units(G, Ppad);
    GG_REQUIRE(J == 1 || J == 2 || J == 4, GG_EINVAL, "k_arnoldi_persist2: vectors too long");
    GG_REQUIRE(G <= kGatherPer * kBlock, GG_EINVAL, "k_arnoldi_persist2: grid beyond the all-gather's reach");
#define GG_P2(JJ)                                                                                             \
    k_arnoldi_persist2<JJ><<<G, kBlock, persist_test_lds(), st>>>(g, zs, i, m, ds, w, V, ldv, H, cs, sn, s, hist, \
                                                                  gran, Ppad / 2, err, xb, elect, seq, um)
    if (J == 1) GG_P2(1);
    else if (J == 2) GG_P2(2);
    else GG_P2(4);
#undef GG_P2
}

}  // namespace gg
