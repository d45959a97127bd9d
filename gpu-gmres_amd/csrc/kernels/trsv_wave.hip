// trsv_wave.hip -- structured-grid wavefront triangular solves: 2D bands, 3D planes, 3D tiles.
#include "device.h"
#include "host.h"

namespace gg {

namespace {

// 2D structured-grid wavefront solve.  Layout (gg_internal.h Wave2D): band =
// 64 grid lines, lane l = line 64*band+l, step t = column i + l; a lane's two
// consecutive steps are adjacent in memory (16 B per array per step pair, 1 KiB
// per wave instruction).
//
// One workgroup per band, 3 + A waves (A = streamed arrays: b, c1, c2 and, for
// a non-unit triangle, the divisor d and its reciprocal):
//  * wave 0 (compute) runs the recurrence.  Each step a lane needs its own
//    previous value (same line, column i-+1) and the neighbour line's value
//    from the previous step, moved in-register with DPP wave_shr/wave_shl; the
//    edge lane keeps the DPP "old" operand, which holds the neighbouring band's
//    value.  Its operands come from LDS a few step pairs ahead of their use,
//    so the recurrence waits on memory at most once per batch; its results go to LDS staging (a global store costs the issuing
//    wave ~50 cycles, an LDS write a few);
//  * wave 2 (writer) stores the compute wave's x from LDS staging to HBM and
//    publishes the band's edge values, one batch behind;
//  * waves 3.. (loaders, one array each) stream HBM -> LDS with LDS-DMA
//    (global_load_lds_dwordx4) into an R-slot ring, each retiring batches with
//    its own counted vmcnt before the barrier (batch j by barrier j);
//  * wave 1 (boundary) polls the neighbouring band's edge values and hands
//    them over through LDS.
// All waves meet at one raw s_barrier per batch (no fence, no drain).
// Band-to-band hand-off (workgroups on different CUs): one 8-byte granule per
// step, bnd[band*T + t], whose payload is the flag (sentinel = not ready).  The
// producing band's writer wave stores the edge values of a batch with one
// relaxed agent-scope (sc1) store; the consumer polls with relaxed agent-scope loads
// and re-arms each granule it read (sc1 sentinel store) for the next launch.
// Every spin is bounded.
//
// Division (non-unit triangles).  x = RN(acc / d) is needed bit-exactly.  The
// IEEE division sequence (div_scale/rcp/fma/div_fmas/div_fixup) is ~70 cycles
// of dependent latency per step; WD_RCP instead uses the host-computed
// reciprocal y = RN(1/d) and two FMA corrections (Markstein):
//   q0 = RN(acc*y); q1 = RN(q0 + RN(acc - d*q0)*y); q2 = RN(q1 + (acc - d*q1)*y)
// q1 is within one ulp of acc/d, so acc - d*q1 is exact and q2 = RN(acc/d)
// (Markstein's theorem; y within half an ulp of 1/d).  The remainders are
// formed as -(d*q - acc) so signed zeros come out as in acc/d.  The theorem
// needs every intermediate in the normal range: the host admits WD_RCP only for
// 2^-100 <= |d| <= 2^100, and the writer wave flags results outside rcp_safe
// (err bit 2), on which the caller repeats the work with WD_HW.
// WD_MUL (gg_set_division(GG_DIV_RCP), tolerance parity): x = RN(acc * y) with
// the streamed y = RN(1/d) in place of d -- within about one ulp of RN(acc/d)
// per row, one dependent multiply instead of five operations, four streamed
// arrays instead of five.  The oracle restates it (orc_set_div_mode) for the
// order-matched checks; the host admits it when every 1/d is finite and normal.
// Steps per batch: one barrier, one boundary hand-over and one LDS-latency
// exposure per batch, so longer is cheaper per step, as far as the LDS budget
// lets the ring hold kWaveRing of them (GG_WAVE_BATCH_UNIT for the unit
// triangle, 3 streams; the non-unit ones stream 4-5 arrays).
#ifndef GG_WAVE_BATCH_UNIT
#define GG_WAVE_BATCH_UNIT 16
#endif
#ifndef GG_WAVE_POLL
#define GG_WAVE_POLL 2
#endif
#ifndef GG_WAVE_BATCH_HW
#define GG_WAVE_BATCH_HW 16
#endif
#ifndef GG_WAVE_BATCH_RCP
#define GG_WAVE_BATCH_RCP 16
#endif
// the compute wave reads a batch's operands after that batch's barrier, kWaveLook
// step pairs ahead of their use
#ifndef GG_WAVE_LOOK
#define GG_WAVE_LOOK 3
#endif
constexpr int kWaveLook = GG_WAVE_LOOK;
// the unit forward solve with the SpMV in its launch looks further ahead
// (round 5, one box each: C2's fused L 96.2 -> 93.8 us at 4 pairs; the U solve
// lost 1.5 us at 4 and the netlist's unfused unit L 2.2 us, so they keep 3)
#ifndef GG_WAVE_LOOK_L
#define GG_WAVE_LOOK_L 4
#endif
constexpr int kWaveLookL = GG_WAVE_LOOK_L;
// the compute wave's LDS traffic is issued in the shadow of each step's DPP shift
#ifndef GG_WAVE_SHADOW
#define GG_WAVE_SHADOW 1
#endif
constexpr bool kWaveShadow = GG_WAVE_SHADOW != 0;
// Ring depth: batches j and j+1 are in LDS at barrier j and kWaveRing-3 more are
// in flight (enough to cover the HBM latency at this stream rate).
#ifndef GG_WAVE_RING
#define GG_WAVE_RING 5
#endif
constexpr int kWaveRing = GG_WAVE_RING;
// One loader wave streaming every array, or one per array.  Every wave with
// loads in flight on a CU delays that CU's hand-off polls (MI355X_MICROARCH.md
// handoff-1to1: the price sits in the consumer CU's memory queue).
#ifndef GG_WAVE_LOADERS
#define GG_WAVE_LOADERS 1
#endif
constexpr int kWaveLoaders = GG_WAVE_LOADERS;
// the writer publishes a batch when the compute wave has staged it (1) or after
// the next batch's barrier (0); the boundary wave passes the barrier before (1)
// or after (0) its re-arm store and look-ahead poll.  Measured on C2 (U solve):
// 0/0 120.4 us, early barrier 123.8, decoupled 191-194 (the writer's LDS polls
// slow the compute wave's LDS traffic) -- so 0/0 for the 2D kernel, while the
// 3D tile kernel, whose bands wait on two sources, gains from both.
#ifndef GG_WAVE_DECOUPLE
#define GG_WAVE_DECOUPLE 0
#endif
// Round 6, re-measured on the per-wave compute loop (C2, one box, alternating,
// profiles/r06/earlybar_ab.txt): the early barrier helps the forward solve (L
// 83.2 -> 81.0 us) and not the backward one (U 81.2 -> 81.7): 2 = forward only
// (0 none, 1 both); C2 4,299 -> 4,339 it/s
#ifndef GG_WAVE_EARLYBAR
#define GG_WAVE_EARLYBAR 2
#endif
// (Measured, not kept, round 5: the 2D boundary wave retrying a batch's
// granules with two polls in flight, s_sleep 0 / 1 / 10 between them: C2 U
// 99.6 -> 102.6-105.6 us, L 95.7 -> 97.8-101.5 us, profiles/r05/stage_ab.txt.)
// GG_WAVE_XCD = X workgroups dealt per band of the backward solve, one running:
// the bands land on 8 / X of the XCDs (8: all on one XCD, 4: alternating over
// two, 2: over four).  Round 5, two compute waves per band, C2 on one box:
// U 99.3 us at 8 -> 97.9 at 4, 98.7 at 2 (profiles/r05/stage_ab.txt r05ab / r05ad)
#ifndef GG_WAVE_XCD
#define GG_WAVE_XCD 4
#endif
// Hand-off through the XCD's own L2 (2D single solves).  GG_WAVE_NG_U
// / GG_WAVE_NG_L = NG > 0 for the backward / forward solve: kWaveCand candidate
// workgroups are dealt per band and band number k of the dependency order runs
// in candidate k * NG / nbands (wave_candidate), so -- workgroups being dealt
// round-robin over the XCDs -- NG contiguous groups of bands share an XCD each;
// every band publishes its XCD (xcc_id) in a word tagged with the launch's
// number, and a writer wave whose consumer band's word names its own XCD
// publishes the edge granules with a plain store (st_plain, device.h) instead
// of the sc1 one.  The protocol never relies on the placement: a consumer
// whose word is not known yet, or names another XCD, gets sc1 stores.
// 0: the placement above (GG_WAVE_XCD; forward: one workgroup per band) and
// sc1 stores only.
#ifndef GG_WAVE_NG_U
#define GG_WAVE_NG_U 0
#endif
#ifndef GG_WAVE_NG_L
#define GG_WAVE_NG_L 2
#endif
constexpr int kWaveCand = 8;                // candidate workgroups per band: one per XCD
static_assert(GG_WAVE_NG_U >= 0 && GG_WAVE_NG_U <= kWaveCand && GG_WAVE_NG_L >= 0 && GG_WAVE_NG_L <= kWaveCand,
              "groups of bands: at most one per candidate");
// the candidate that runs band number k (of nbands, in dependency order) with ng groups
__host__ __device__ constexpr int wave_candidate(int nbands, int ng, int k)
{
    return (int)((long long)k * ng / nbands);
}
// groups of a direction's 2D single solve (0: no dealing by groups) and the
// workgroups its launch holds per band -- the kernel and its launchers both
// take them from here
constexpr int wave_groups(bool fwd) { return fwd ? GG_WAVE_NG_L : GG_WAVE_NG_U; }
constexpr int wave_deal(bool fwd) { return wave_groups(fwd) > 0 ? kWaveCand : fwd ? 1 : GG_WAVE_XCD; }
// The fused SpMV + L launch deals by groups for the unit L's fused rows (ILU(0)
// grids) only: the split engine's launch divides in its SpMV blocks' gathers,
// and with the CUs that the candidates take from them its bands wait for b
// (bench.py --workload pg, one run each: 4,169 -> 4,100 it/s with the dealing).
constexpr int wave_deal_fs(int div) { return div == WD_UFMA ? wave_deal(true) : 1; }
// CUs per band that the launch's SpMV blocks leave free
#ifndef GG_WAVE_FS_SPARE
#define GG_WAVE_FS_SPARE (wave_deal_fs(WD_UFMA))
#endif
// Redundant compute waves: GG_WAVE_NC waves (on distinct SIMDs) run the same
// recurrence on the same operands -- bit-identical values -- and wave c stages
// only the step pairs kk with kk % NC == c for the writer wave.  A single
// wave's LDS store path runs at half rate (MI355X_MICROARCH.md LDS table:
// stores from one wave), so the pair's ds_write_b128 (~26 cycles) sat on the
// recurrence: C2 trace 44 cycles per step with it, 33 with no staging at all
// (timing bound, GG_WAVE_NOSTAGE; C2 4,123 -> 4,350 it/s on one box).
// Measured on one box (round 5, profiles/r05/stage_ab.txt): NC = 1 / 2 / 3 / 4
// 3,723 / 3,787 / 3,700 / 3,689 it/s (more waves: more LDS reads and a later
// barrier), so 2.  Not kept: four ds_write_addtid_b32 per pair instead of the
// b128 (one data dword, no address): 53 cycles per step -- a single wave's
// addtid stores run at a fraction of their rate.  Nor (round 5, C2 one box,
// profiles/r05/stage_ab.txt): the compute waves storing x themselves (one
// global_store_dwordx4 per pair) and handing only the edge lane's batch to the
// writer through LDS: 3,408 / 3,440 it/s (NC 2 / 1) against 3,773 -- stores
// from one active lane cost the store path what full ones do (8 b128 at the
// batch end: 551 cycles to the barrier).
#ifndef GG_WAVE_NC
#define GG_WAVE_NC 2
#endif
constexpr int kWaveNC = GG_WAVE_NC;
// diagnostics only (timing bound, wrong results): no x staging at all
#ifndef GG_WAVE_NOSTAGE
#define GG_WAVE_NOSTAGE 0
#endif

template <int DIV, bool D3 = false, int S = 1>
struct WaveCfg {
    // streamed arrays: b, c1, c2 (, d (, RN(1/d))); a skewed 2D grid (ILU(S-1))
    // adds the fill coefficients of offsets nx-1 .. nx-S+1; a 3D grid adds the
    // plane coefficient c0 and the previous plane's x
    static constexpr int AE = (DIV == WD_UNIT || DIV == WD_UFMA) ? 3 : DIV == WD_RCP ? 5 : 4;   // first fill array (WD_MUL / WD_SFMA stream y as d)
    static constexpr int A2 = AE + (S - 1);
    static constexpr int A = A2 + (D3 ? 2 : 0);
    static constexpr int B16 = (DIV == WD_UNIT || DIV == WD_UFMA) ? GG_WAVE_BATCH_UNIT
                             : DIV == WD_RCP  ? GG_WAVE_BATCH_RCP
                                              : GG_WAVE_BATCH_HW;
    // steps per batch: 8 where 16-step slots of A arrays would not leave room for 3 slots
    static constexpr int B = (B16 == 16 && 3 * A * 8 * 64 + 64 + 2 * 8 * 64 > 150 * 1024 / 16) ? 8 : B16;
    static constexpr int PBN = B / 2;                                     // step pairs per batch
    static constexpr int SLOT = A * PBN * 64;                            // double2 per ring slot
    // loader waves: GG_WAVE_LOADERS where it divides the arrays (2D, unskewed),
    // each streaming A / LOADERS of them with its own vmcnt budget
    static constexpr int LOADERS = (!D3 && S == 1 && kWaveLoaders > 1 && A % kWaveLoaders == 0) ? kWaveLoaders : 1;
    static constexpr int NA = A / LOADERS;                              // arrays per loader wave
    static constexpr int NPER = NA * PBN;                               // DMA instructions per batch per loader
    // ring slots: kWaveRing, at most what fits 150 KiB of LDS beside the boundary
    // values and the x staging, and at most what the 6-bit vmcnt can count
    static constexpr int RFIT = (150 * 1024 / 16 - 64 - 2 * PBN * 64) / SLOT;
    static constexpr int RVM = 2 + 63 / NPER;
    static constexpr int R = kWaveRing < RFIT ? (kWaveRing < RVM ? kWaveRing : RVM) : (RFIT < RVM ? RFIT : RVM);
    static constexpr int NC = kWaveNC;                                  // redundant compute waves
    static constexpr int THREADS = (2 + NC + LOADERS) * 64;             // compute(s), boundary, writer, loaders
    static constexpr int LDS2 = R * SLOT + 64 + 2 * PBN * 64;            // ring, boundary, x staging
    static_assert(R >= 3 && (R - 2) * NPER <= 63, "ring depth vs vmcnt range");
    static_assert(B == 8 || B == 16, "batch");
    static_assert(kWaveTAlign % (B * GG_WAVE_POLL) == 0, "batches per band must be a multiple of the poll depth");
    static_assert(!D3 || LOADERS == 1, "3D grids stream every array from one loader wave");
    static_assert(S >= 1 && S <= 3 && (S == 1 || (!D3 && LOADERS == 1)), "skew: 2D, one loader");
    static_assert(kWaveLook >= 1 && kWaveLook <= PBN && kWaveLookL >= 1 && kWaveLookL <= PBN, "lookahead");
    static_assert(LDS2 * 16 <= 160 * 1024, "LDS budget");
};

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void gbl_void_t;

// s_waitcnt immediate: wait until <= n vector-memory ops are outstanding (gfx9)
__host__ __device__ constexpr int vm_wait(int n)
{
    return (n & 15) | (7 << 4) | (0xF << 8) | (((n >> 4) & 3) << 14);
}
// wait until at most max(min(after, K), 0) batches of NPER instructions are in flight
template <int K, int NPER>
__device__ __forceinline__ void vm_wait_batches(int after)
{
    if constexpr (K == 0) {
        __builtin_amdgcn_s_waitcnt(vm_wait(0));
    } else {
        static_assert(K * NPER <= 63, "vmcnt is 6 bits");
        if (after >= K) __builtin_amdgcn_s_waitcnt(vm_wait(K * NPER));
        else vm_wait_batches<K - 1, NPER>(after);
    }
}

__device__ __forceinline__ void raw_barrier() { asm volatile("s_barrier" ::: "memory"); }

// 64-bit DPP lane shift whose out-of-range lane keeps `old`
template <int CTRL>
__device__ __forceinline__ double dpp_shift_old(double v, double old)
{
    int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, 0xf, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// WD_RCP's range condition, checked on the results x (by the writer wave, off
// the recurrence): with 2^-100 <= |d| <= 2^100, |x| in [2^-800, 2^800] keeps
// |acc| = |x d| inside [2^-900, 2^900], where every intermediate of the two
// corrections is normal.  x == 0 comes from acc == 0, or from a quotient below
// 2^-1074 that both roundings flush alike except within one subnormal ulp.
__device__ __forceinline__ bool rcp_safe(double v)
{
    const double a = __builtin_fabs(v);
    return v == 0.0 || (a >= 0x1p-800 && a <= 0x1p800);
}

// loader wave: batch j -> ring slot j % R; batch j landed by barrier j
template <bool FWD, int R, int SLOT, int NA, int PBN, int SC1 = -1>
__device__ __forceinline__ void wave_loader(const double2 *const *src, double2 *lds, int np, int nbatch,
                                            long long *tr = nullptr)
{
    // array SC1 (a 3D grid's previous-plane x, written by another workgroup in
    // this launch) is read write-through coherent (sc1: cache policy 16)
    constexpr int PB = PBN * 64;                // double2 per array per slot
    auto issue = [&](int j) {
        double2 *slot = lds + (j % R) * SLOT;
#pragma unroll
        for (int a = 0; a < NA; a++) {
            if (a == SC1) continue;
#pragma unroll
            for (int kk = 0; kk < PBN; kk++) {
                const int p = j * PBN + kk;
                const long long q = (long long)(FWD ? p : np - 1 - p) * 64;
                __builtin_amdgcn_global_load_lds((gbl_void_t *)(src[a] + q),
                                                 (lds_void_t *)(slot + a * PB + kk * 64), 16, 0, 0);
            }
        }
        if constexpr (SC1 >= 0) {
#pragma unroll
            for (int kk = 0; kk < PBN; kk++) {
                const int p = j * PBN + kk;
                const long long q = (long long)(FWD ? p : np - 1 - p) * 64;
                __builtin_amdgcn_global_load_lds((gbl_void_t *)(src[SC1] + q),
                                                 (lds_void_t *)(slot + SC1 * PB + kk * 64), 16, 0, 16);
            }
        }
    };
    for (int j = 0; j < R - 1 && j < nbatch; j++) issue(j);
    for (int j = 0; j < nbatch; j++) {
        // batch j must have landed; the ones after it may stay in flight
        const int issued = j + R - 1 < nbatch ? j + R - 1 : nbatch;
        vm_wait_batches<R - 2, NA * PBN>(issued - (j + 1));
        if (tr && (threadIdx.x & 63) == 0) tr[j] = (long long)__builtin_amdgcn_s_memrealtime();   // diagnostics
        raw_barrier();                          // slot (j-1) % R is free from here on
        if (j + R - 1 < nbatch) issue(j + R - 1);
    }
}

// The SpMV fused into the forward solve's launch (GG_FUSE_SPMV, k_trsv_wave2d_spmv):
// b = A v is produced by extra workgroups of the same launch (blocks >= nbands)
// while the bands run.  Slices (64 layout rows, the sliced-ELL copy of A) are
// taken kFsGroup at a time in band-major order, each row summed exactly as
// k_spmv_sell sums it (entry order, no contraction), stored write-through
// (agent scope) and counted per band once drained; a band's loader wave waits
// for its band's count before its first batch (no DMA in flight then), re-arms
// the counter and streams b with the coherent (sc1) policy.  The SpMV blocks
// never wait on anything and take the LOW block indices, so they are dispatched
// before the bands that wait on them: with more bands than resident slots the
// SpMV blocks still finish and the bands run in dispatch order, each waiting
// only on blocks dispatched before it (with the bands first, a grid
// of nbands >= resident slots would spin on never-dispatched SpMV blocks).
struct FusedSpmv {
    const int *sptr = nullptr, *sci = nullptr;
    const double *sv = nullptr, *v = nullptr;
    double *w = nullptr;                    // = the solve's b
    unsigned long long *cnt = nullptr;      // per slice group: 1 = stored (0 between launches)
    const double *ydiv = nullptr;           // split engine: row divisors (k_spmv_sell's YDIV)
    const double *xdiv = nullptr;           // split engine: v[c] / xdiv[c] per gathered term (k_spmv_sell's XDIV)
    int n = 0;                              // rows of A (layout space)
    int ns = 0;                             // SpMV blocks: blockIdx < ns, the bands after them
};
// slices per group: C2 fused L 92.5 / 87.0 / 85.8 us at 8 / 4 / 2 (a group's
// chain is shorter with fewer loads per lane; profiles/r03/r03_fs_knobs.txt)
constexpr int kFsGroup = 2;                 // (kWaveTAlign is a multiple)

template <bool XD>
__device__ __forceinline__ void fused_spmv_groups(const FusedSpmv &fs, int nbands, int T, int nwv)
{
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int NW = fs.ns * nwv;
    const int gpb = T / kFsGroup;
    const int ngroups = nbands * gpb;
    for (int q = (int)blockIdx.x * nwv + wv; q < ngroups; q += NW) {
        const int s0 = q * kFsGroup;
        int off[kFsGroup], wd[kFsGroup];
        int wmax = 0;
#pragma unroll
        for (int j = 0; j < kFsGroup; j++) {
            off[j] = fs.sptr[s0 + j];
            wd[j] = (fs.sptr[s0 + j + 1] - off[j]) >> 6;
            wmax = wd[j] > wmax ? wd[j] : wmax;
        }
        double acc[kFsGroup];
#pragma unroll
        for (int j = 0; j < kFsGroup; j++) acc[j] = 0.0;
        for (int k0 = 0; k0 < wmax; k0 += 8) {
            int c[kFsGroup][8];
            double a[kFsGroup][8], xv[kFsGroup][8];
#pragma unroll
            for (int j = 0; j < kFsGroup; j++)
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (k0 + k < wd[j]) {
                        c[j][k] = __builtin_nontemporal_load(fs.sci + off[j] + lane + (k0 + k) * 64);
                        a[j][k] = __builtin_nontemporal_load(fs.sv + off[j] + lane + (k0 + k) * 64);
                    }
#pragma unroll
            for (int j = 0; j < kFsGroup; j++)
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (k0 + k < wd[j] && c[j][k] >= 0) xv[j][k] = fs.v[c[j][k]];
            if constexpr (XD) {
                double dv[kFsGroup][8];
#pragma unroll
                for (int j = 0; j < kFsGroup; j++)
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        if (k0 + k < wd[j] && c[j][k] >= 0) dv[j][k] = fs.xdiv[c[j][k]];
#pragma unroll
                for (int j = 0; j < kFsGroup; j++)
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        if (k0 + k < wd[j] && c[j][k] >= 0) xv[j][k] = xv[j][k] / dv[j][k];
            }
#pragma unroll
            for (int j = 0; j < kFsGroup; j++)
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (k0 + k < wd[j] && c[j][k] >= 0) acc[j] += a[j][k] * xv[j][k];
        }
#pragma unroll
        for (int j = 0; j < kFsGroup; j++) {
            const int r = (s0 + j) * 64 + lane;
            if (r < fs.n) {
                const double o = fs.ydiv ? acc[j] / fs.ydiv[r] : acc[j];
                st_agent(reinterpret_cast<unsigned long long *>(fs.w) + r, (unsigned long long)__double_as_longlong(o));
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the group's rows stored
        if (lane == 0) st_agent(fs.cnt + q, 1ull);          // one word per group: no contention
    }
}
// xdiv (the split engine's D_r^-1 pass folded into the gathers, as
// k_spmv_sell<.., XDIV>): one uniform branch, the loops unchanged otherwise
__device__ __forceinline__ void fused_spmv_role(const FusedSpmv &fs, int nbands, int T, int nwv)
{
    if (fs.xdiv) fused_spmv_groups<true>(fs, nbands, T, nwv);
    else fused_spmv_groups<false>(fs, nbands, T, nwv);
}

// IL: the in-line term (|offset| = 1) comes first in the row's canonical order,
// then the line term -- the split (ILU++) U factor's ascending-column rows
// (MyILUPP::HostPrecond_right, src/preconditioner.cu:1117-1137).
// FS: the SpMV fused into the launch (see FusedSpmv; forward unskewed 2D only).
// BT: a batched launch (the many-RHS solve) -- zS scenarios of nbands
// workgroups each; scenario sc's b, x and hand-off granules (with its dummies)
// lie sc * zs bytes after scenario 0's, its control block likewise (the gate).
// zmap 0: workgroup = band * zS + sc (workgroups being dealt round-robin over
// the XCDs, a scenario's bands share an XCD when zS is a multiple of 8, so its
// hand-offs stay in one L2); zmap 1: workgroup = sc * nbands + band (band b of
// every scenario on one XCD: the coefficient streams shared in its L2).
template <bool FWD, int DIV, bool TRACE, bool D3, int S, bool IL, bool FS, bool BT = false>
__device__ __forceinline__ void trsv_wave2d_body(
    Gate g, int T, int nbands, const double *__restrict__ b, const double *__restrict__ c1,
    const double *__restrict__ c2, const double *__restrict__ dv, const double *__restrict__ rv,
    double *__restrict__ x, unsigned long long *bnd, int *err, long long *trace,
    int nz, long long P2, const double *__restrict__ c0, unsigned long long *prog,
    const double *__restrict__ ce1, const double *__restrict__ ce2, const FusedSpmv &fs,
    int zS = 1, long long zs = 0, int zmap = 0, unsigned long long *xw = nullptr, unsigned long long xseq = 0)
{
    using C = WaveCfg<DIV, D3, S>;
    // LDS work in the lane shift's shadow -- not for the unit L's fused rows,
    // whose step is one FMA after the shift: there the pair's reads and staging
    // write go after the pair (C2 fused L 86.7 -> 84.5 us, netlist L 91.5 ->
    // 90.4; the other forms keep it: the exact unit L 88.9 -> 90.3 without)
    constexpr bool SH = kWaveShadow && DIV != WD_UFMA;
    static_assert(!FS || (FWD && !D3 && S == 1 && !TRACE), "fused SpMV: forward 2D");
    static_assert(!IL || (S == 1 && !D3), "in-line-first rows: unskewed 2D grids");
    constexpr bool FM = DIV == WD_UFMA || DIV == WD_SFMA;     // GG_DIV_FMA rows
    static_assert(!FM || (!D3 && !IL), "fused rows: 2D grids (one order for both IL)");
    static_assert(!(TRACE && S > 1), "no trace for skewed grids");
    constexpr int PB = C::PBN * 64;            // double2 per array per slot
    static_assert(!(D3 && TRACE), "no trace for 3D grids");
    static_assert(!BT || (!FS && !D3 && !TRACE), "batched: 2D, separate SpMV, no trace");
    if (!BT && gated(g)) return;
    int bid = (int)blockIdx.x;                  // this workgroup among the bands
    if constexpr (BT) {
        const int sc = zmap == 0 ? bid % zS : bid / nbands;
        bid = zmap == 0 ? bid / zS : bid % nbands;
        if (gated_z(g, zs, sc)) return;
        b = zp(b, zs, sc);
        x = zp(x, zs, sc);
        bnd = zp(bnd, zs, sc);
    }
    if constexpr (FS) {
        if (bid < fs.ns) {
            fused_spmv_role(fs, nbands, T, C::THREADS / 64);
            return;
        }
        bid -= fs.ns;
    }
    // one LDS object: data ring [R][A][C::PBN][64] double2, 2 x 64 boundary values
    // (lanes 0..C::B-1 of each half are used), x staging [2][C::PBN][64]
    __shared__ double2 lds[C::LDS2];
    __shared__ int xdone;                       // batches the compute wave has staged (GG_WAVE_DECOUPLE)
    double2 *ring = lds;                        // ring | boundary | x staging
    double *bring = reinterpret_cast<double *>(lds + C::R * C::SLOT);
    double2 *xbuf = lds + C::R * C::SLOT + 64;
    if (threadIdx.x == 0) xdone = 0;            // read only after the first barrier
    int seq = 0;                                // batches this workgroup has run (uniform)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int np = T / 2;                       // step pairs per band
    const int nbatch = T / C::B;          // T is a multiple of kWaveTAlign
    constexpr int plane = FWD ? 63 : 0;     // lane whose values the next band needs
    // Tasks: (plane, band) in dependency order, a workgroup takes every
    // gridDim.x-th (2D: one band per workgroup, nz = 1).  A 3D task also needs
    // the previous plane's x (same band): its writer publishes prog[] =
    // batches stored, the boundary wave polls it, the loader streams it.
    // GG_WAVE_XCD = X > 1 (2D backward solve): the launch has X workgroups per
    // band and only every X-th runs one, so that (workgroups being dealt
    // round-robin over the XCDs) the bands share one XCD and its L2 --
    // placement is for speed only, the hand-off protocol is the same.
    // Measured on C2: U 121.0 -> 117.9 us, while L (3 streamed arrays) slows
    // 88.9 -> 90.0 us (round 3, re-measured: 89.4 / 90.3 -> 89.9 / 90.4 us), so
    // the forward solve keeps one workgroup per band.
    // GG_WAVE_NG_U / _L = NG > 0: kWaveCand workgroups per band, the one of the
    // band's group running it (the fused SpMV's launch too: its other
    // candidates exit, the SpMV blocks keep the low indices).
    constexpr bool GRP = !D3 && !BT && !(FS && wave_deal_fs(DIV) == 1);
    constexpr int NG = GRP ? wave_groups(FWD) : 0;
    constexpr int XS = (D3 || BT) ? 1 : FS ? wave_deal_fs(DIV) : wave_deal(FWD);
    if (XS > 1 && bid % XS != (NG > 0 ? wave_candidate(nbands, NG, bid / XS) : 0)) return;
    const int blk = bid / XS;
    // the hand-off through the XCD's L2: compiled for NG > 0, run where the
    // launcher passes the bands' XCD words
    constexpr bool L2H = NG > 0;
    const int ntask = nz * nbands;
    for (int task = blk; task < ntask; task += ((FS || BT) ? nbands : (int)gridDim.x / XS)) {
    const int kq = task / nbands, bq = task % nbands;
    const int band = FWD ? bq : (nbands - 1 - bq);
    const int kp = FWD ? kq : (nz - 1 - kq);    // plane
    const bool has_src = FWD ? (band > 0) : (band < nbands - 1);
    const bool is_prod = FWD ? (band < nbands - 1) : (band > 0);
    const bool has_prev = D3 && (FWD ? kp > 0 : kp < nz - 1);
    const long long boff = (long long)band * np * 64 + lane + (long long)kp * (P2 / 2);   // double2 units
    const long long prev_off = (FWD ? -1 : 1) * (P2 / 2);                                // previous plane
    unsigned long long *pub = bnd + ((long long)kp * nbands + band) * T;
    unsigned long long *prog_mine = D3 ? prog + (long long)kp * nbands + band : nullptr;
    unsigned long long *prog_prev = has_prev ? prog + (long long)(FWD ? kp - 1 : kp + 1) * nbands + band : nullptr;
    constexpr int NC = C::NC;                   // waves [0, NC) compute, NC boundary, NC + 1 writer, loaders
    static_assert(NC >= 1 && NC <= 4 && (NC == 1 || !GG_WAVE_DECOUPLE), "redundant compute waves");
    if (wave >= NC + 2) {
        // ------------------------------------------------ loader wave(s)
        const int li = wave - NC - 2;           // this loader's arrays: [li * NA, (li + 1) * NA)
        const double2 *src[7] = {reinterpret_cast<const double2 *>(b) + boff,
                                 reinterpret_cast<const double2 *>(c1) + boff,
                                 reinterpret_cast<const double2 *>(c2) + boff,
                                 reinterpret_cast<const double2 *>(dv) + boff,
                                 reinterpret_cast<const double2 *>(rv) + boff,
                                 nullptr, nullptr};
        if constexpr (S >= 2) src[C::AE] = reinterpret_cast<const double2 *>(ce1) + boff;
        if constexpr (S >= 3) src[C::AE + 1] = reinterpret_cast<const double2 *>(ce2) + boff;
        if constexpr (D3) {
            // the plane coefficient and the previous plane's x (zeros on the
            // first plane, where c0 is 0) follow the 2D arrays
            src[C::A2] = reinterpret_cast<const double2 *>(c0) + boff;
            src[C::A2 + 1] = reinterpret_cast<const double2 *>(has_prev ? x : c0) + boff + (has_prev ? prev_off : 0);
        }
        if constexpr (D3) {
            // the prologue streams batches 0..R-2 before the boundary wave has
            // checked anything: wait here for the previous plane to store them
            // (no DMA is in flight yet, so a blocking poll is free)
            if (has_prev) {
                const unsigned long long need = (unsigned long long)(C::R - 1 < nbatch ? C::R - 1 : nbatch);
                int spins = 0;
                while (ld_agent(prog_prev) < need) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > kSpinLimit) {
                        if (lane == 0) atomicOr(err, 1);
                        break;
                    }
                }
            }
        }
        if (FS && li == 0) {
            // this band's b rows all stored by the SpMV blocks (no DMA in flight
            // yet: a blocking poll is free); the counter is re-armed after the
            // stream (a store in flight would upset the loader's vmcnt count)
            // -- by the loader of b (array 0) alone
            const int gpb = T / kFsGroup;
            const unsigned long long *fl = fs.cnt + (long long)band * gpb;
            auto all_stored = [&]() {
                bool ok = true;
                for (int k = lane; k < gpb; k += 64) ok &= ld_agent(fl + k) != 0ull;
                return __all(ok);
            };
            int spins = 0;
            while (!all_stored()) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > kSpinLimit) {
                    if (lane == 0) atomicOr(err, 1);
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        if constexpr (C::LOADERS == 1) {
            wave_loader<FWD, C::R, C::SLOT, C::A, C::PBN, D3 ? C::A2 + 1 : FS ? 0 : -1>(src, ring, np, nbatch);
        } else if (li == 0) {
            wave_loader<FWD, C::R, C::SLOT, C::NA, C::PBN, FS ? 0 : -1>(src, ring, np, nbatch);
        } else {
            wave_loader<FWD, C::R, C::SLOT, C::NA, C::PBN>(src + li * C::NA, ring + li * C::NA * PB, np, nbatch);
        }
        if (FS && li == 0) {
            const int gpb = T / kFsGroup;
            for (int k = lane; k < gpb; k += 64) st_agent(fs.cnt + (long long)band * gpb + k, 0ull);   // re-arm
        }
        raw_barrier();                      // final barrier (the writer drains the last batch)
        continue;
    }
    if (wave == NC + 1) {
        // ------------------------------------------------ writer wave
        // After barrier bi+1 the compute wave's x of batch bi sits in xbuf[bi & 1]:
        // store it to HBM and publish the edge lane's values of the batch as
        // hand-off granules (lanes 0..C::B-1, one coalesced sc1 store).
        // 3D: x is stored write-through (sc1) and, once a batch's stores have
        // drained (checked one batch later, off the critical path), counted in
        // prog_mine for the next plane.
        // GG_WAVE_DECOUPLE: batch bi is published as soon as the compute wave
        // has staged it (LDS counter xdone), not after barrier bi+1, which
        // also waits for this band's boundary values of batch bi+1: a band's
        // upstream must not hold back what it hands downstream.
        double2 *X2 = reinterpret_cast<double2 *>(x) + boff;
        [[maybe_unused]] bool bad = false;  // WD_RCP range guard (see rcp_safe)
        // L2H: this band's XCD goes into its word (sc1, tagged with the launch's
        // number: a word left by an earlier or a gated launch reads as unknown);
        // the consumer band's word is requested here and looked at when the first
        // batch is published, then once per batch until it carries this launch's
        // tag -- no spin, and an unknown consumer simply gets sc1 stores.  local:
        // the consumer runs on this XCD, so its sc1 polls are served by the L2
        // that a plain store stops in.
        [[maybe_unused]] unsigned long long cword = 0;
        [[maybe_unused]] const unsigned long long *cwp = nullptr;
        [[maybe_unused]] unsigned myx = 0;
        [[maybe_unused]] bool cknown = false, local = false;
        [[maybe_unused]] long long nlocal = 0;
        if constexpr (L2H || TRACE) myx = xcc_id();
        if constexpr (L2H) {
            if (xw) {
                if (lane == 0) st_agent(xw + (long long)band * kWaveXcdWord, (xseq << 4) | 8ull | myx);
                if (is_prod) {
                    cwp = xw + (long long)(FWD ? band + 1 : band - 1) * kWaveXcdWord;
                    cword = ld_agent(cwp);
                }
            }
        }
        for (int bi = 0; bi <= nbatch; bi++) {
            if (!GG_WAVE_DECOUPLE || bi == 0) raw_barrier();
            if (bi == 0) continue;
            const int pb = bi - 1;
            if constexpr (L2H) {
                if (cwp && !cknown) {
                    const unsigned long long cw =
                        (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)cword) |
                        ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(cword >> 32)) << 32);
                    if ((cw >> 4) == xseq && (cw & 8ull)) {
                        cknown = true;
                        local = (unsigned)(cw & 7ull) == myx;
                    } else {
                        cword = ld_agent(cwp);      // looked at with the next batch
                    }
                }
            }
            if constexpr (GG_WAVE_DECOUPLE) {
                while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&xdone, __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_WORKGROUP)) <= seq + pb)
                    __builtin_amdgcn_s_sleep(1);
            }
            if constexpr (D3) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // batches < pb stored
                if (lane == 0 && pb > 0) st_agent(prog_mine, (unsigned long long)pb);
            }
            const double2 *xb = xbuf + (pb & 1) * PB;
            // the hand-off granules first: they are on the critical path, x is not
            const int tt = lane & (C::B - 1);
            const double e = reinterpret_cast<const double *>(xb + (tt >> 1) * 64 + plane)
                [FWD ? (tt & 1) : 1 - (tt & 1)];
            if (is_prod && lane < C::B) {
                const int t = FWD ? pb * C::B + tt : (T - 1) - (pb * C::B + tt);
                if (L2H && local) st_plain(pub + t, (unsigned long long)__double_as_longlong(e));
                else st_agent(pub + t, (unsigned long long)__double_as_longlong(e));
            }
            if constexpr (TRACE) nlocal += (L2H && local && is_prod) ? 1 : 0;
            double2 v[C::PBN];
#pragma unroll
            for (int kk = 0; kk < C::PBN; kk++) v[kk] = xb[kk * 64 + lane];
#pragma unroll
            for (int kk = 0; kk < C::PBN; kk++) {
                const int p = pb * C::PBN + kk;
                double2 *dst = X2 + (long long)(FWD ? p : np - 1 - p) * 64;
                if constexpr (D3) {
                    st_sc1_16(dst, v[kk]);
                } else {
                    *dst = v[kk];
                }
                if constexpr (DIV == WD_RCP) bad |= !rcp_safe(v[kk].x) || !rcp_safe(v[kk].y);
            }

            if (TRACE && lane == 0)
                trace[(long long)band * (3 * nbatch + 8) + nbatch + 8 + pb] =
                    (long long)__builtin_amdgcn_s_memrealtime();
            if constexpr (GG_WAVE_DECOUPLE) raw_barrier();     // barrier bi (the last: the final one)
        }
        seq += nbatch;
        if constexpr (TRACE) {
            // the band's XCD + 1, the groups compiled in, the batches published
            // with plain stores (ggmres.h, gg_trace_precond)
            if (lane == 0)
                trace[(long long)band * (3 * nbatch + 8) + nbatch + 7] =
                    (long long)(myx + 1) | ((long long)NG << 4) | (nlocal << 8);
        }
        if constexpr (D3) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) st_agent(prog_mine, (unsigned long long)nbatch);
        }
        if constexpr (DIV == WD_RCP) {
            if (__any(bad) && lane == 0) atomicOr(err, 2);
        }
        continue;
    }
    if (wave == NC) {
        // ------------------------------------------------ boundary wave
        // Before barrier bi it places batch bi's values in bring[bi & 1].  Step
        // t of this band's edge lane needs the source band's step t -+ 63.  Polls
        // are pipelined kPoll batches deep (one register per ring position): the
        // load for batch bi+kPoll is issued right after batch bi is handed over,
        // so in steady state a batch's granules have arrived when it is checked.
        // Every memory op is issued by all lanes (lanes with nothing to do use
        // the dummy granules after the bands: 64 zeros to read, 64 to write),
        // which keeps the vmcnt arithmetic exact.
        constexpr int kPoll = GG_WAVE_POLL;
        // the barrier before (EB) or after the re-arm store and look-ahead poll
        constexpr bool EB = GG_WAVE_EARLYBAR == 1 || (GG_WAVE_EARLYBAR == 2 && FWD);
        // 3D: lane 32 polls the previous plane's progress instead: before
        // barrier bi it must have stored the batches the loader streams after
        // it (up to bi + R - 1); its word is never re-armed here, but reset to
        // 0 when this task is done (the producer has finished by then).
        unsigned long long *src = bnd + ((long long)kp * nbands + (FWD ? band - 1 : band + 1)) * T;
        // this workgroup's dummy granules (64 zeros to read, 64 write-only words)
        unsigned long long *dummy_ld = bnd + (long long)nz * nbands * T + (long long)blk * 128 + lane;
        unsigned long long *dummy_st = dummy_ld + 64;
        constexpr int kProgLane = 32;
        const bool prog_lane = has_prev && lane == kProgLane;
        auto gaddr = [&](int bj) {
            const int t = FWD ? bj * C::B + lane : (T - 1) - (bj * C::B + lane);
            const int gi = FWD ? t + (64 * S - 1) : t - (64 * S - 1);     // the neighbour's edge lane
            const bool need = has_src && lane < C::B && bj < nbatch && gi >= 0 && gi < T;
            return need ? src + gi : (unsigned long long *)nullptr;
        };
        auto poll_addr = [&](int bj) -> unsigned long long * {
            if (prog_lane) return prog_prev;
            unsigned long long *ga = gaddr(bj);
            return ga ? ga : dummy_ld;
        };
        auto ready = [&](unsigned long long w, int bj) {
            if (prog_lane) return w >= (unsigned long long)(bj + C::R < nbatch ? bj + C::R : nbatch);
            return w != kSentinel;
        };
        // the prologue mirrors the steady-state issue order (re-arm store, poll)
        // so the same vmcnt holds in every iteration
        unsigned long long v[kPoll];
#pragma unroll
        for (int u = 0; u < kPoll; u++) {
            if (u > 0) st_agent(dummy_st, kSentinel);
            v[u] = ld_agent(poll_addr(u));
        }
        bool dead = false;
        long long bw_spins = 0, bw_cyc = 0;     // TRACE: poll retries, cycles in retry loops
        for (int bi0 = 0; bi0 < nbatch; bi0 += kPoll) {     // nbatch is a multiple of kPoll
#pragma unroll
            for (int u = 0; u < kPoll; u++) {
                const int bi = bi0 + u;
                unsigned long long *ga = gaddr(bi);
                // oldest poll done: after it come kPoll-1 loads and kPoll-1 re-arm stores
                __builtin_amdgcn_s_waitcnt(vm_wait(2 * (kPoll - 1)));
                int spins = 0;
                const long long tw = TRACE ? (long long)__builtin_amdgcn_s_memtime() : 0;
                while (!dead && !__all(ready(v[u], bi))) {
                    __builtin_amdgcn_s_sleep(1);
                    v[u] = ld_agent(poll_addr(bi));
                    if (++spins > kSpinLimit) {
                        dead = true;
                        if (lane == 0) atomicOr(err, 1);
                    }
                    __builtin_amdgcn_s_waitcnt(vm_wait(0));
                }
                if constexpr (TRACE) {
                    bw_spins += spins;
                    if (spins) bw_cyc += (long long)__builtin_amdgcn_s_memtime() - tw;
                    if (lane == 0)
                        trace[(long long)band * (3 * nbatch + 8) + 2 * nbatch + 8 + bi] =
                            (long long)__builtin_amdgcn_s_memrealtime();
                }
                bring[(bi & 1) * 64 + lane] = __longlong_as_double((long long)v[u]);
                if constexpr (EB) {
                    // hand the values over first, then re-arm and poll ahead
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    raw_barrier();
                }
                st_agent(ga ? ga : dummy_st, kSentinel);       // re-arm for the next launch
                v[u] = ld_agent(poll_addr(bi + kPoll));
                if constexpr (!EB) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    raw_barrier();
                }
            }
        }
        raw_barrier();                      // final barrier (the writer drains the last batch)
        if (TRACE && lane == 0) {
            long long *trb = trace + (long long)band * (3 * nbatch + 8);
            trb[nbatch + 5] = bw_spins;
            trb[nbatch + 6] = bw_cyc;
        }
        if (prog_lane) {
            __builtin_amdgcn_s_waitcnt(vm_wait(0));
            st_agent(prog_prev, 0ull);              // re-arm for the next launch
        }
        continue;
    }

    // ---------------------------------------------------- compute wave(s)
    // One copy of the loop per compute wave, its share of the staging (pairs
    // kk with kk % NC == cw) a compile-time choice: a run-time test of the
    // wave index put a scalar branch around every staging store, splitting
    // the scheduled pair into basic blocks (C2 L / U 85 -> 93 / 97 us on one
    // box, profiles/r05/r05_vs_r04/)
    auto compute_wave = [&](auto cw_tag) {
    constexpr int cw = decltype(cw_tag)::value;
    constexpr int ctrl = FWD ? 0x138 : 0x130;   // wave_shr:1 / wave_shl:1
    long long *tr = TRACE && cw == 0 ? trace + (long long)band * (3 * nbatch + 8) : nullptr;
    long long ph[4] = {0, 0, 0, 0};     // TRACE: barrier wait, top->step0, step0->last, last->end
    long long t_top = 0;
    double xp = 0.0;                        // this lane's previous step value
    double xh1 = 0.0, xh2 = 0.0;            // skew > 1: the neighbour line's values 2 and 3 steps back
    // Operands of the current batch in registers, read kWaveLook step pairs
    // ahead of their use; the boundary values are read first (LDS returns in
    // order and they are needed at the batch's first step).
    double2 rg[C::PBN][C::A];
    constexpr int LK = (FS && (DIV == WD_UNIT || DIV == WD_UFMA)) ? kWaveLookL : kWaveLook;
    // one step pair's x into staging half h, pair kk (.x = the value at the
    // lower memory address)
    auto stage = [&](int h, int kk, double vx, double vy) {
        if constexpr (!GG_WAVE_NOSTAGE) {
            if (kk % NC == cw) xbuf[h * PB + kk * 64 + lane] = make_double2(vx, vy);
        }
    };
    raw_barrier();                          // barrier 0: batch 0 is in LDS
    for (int bi = 0; bi < nbatch; bi++) {
        if (bi > 0) {
            // x staging writes of batch bi-1 complete before the barrier (writer)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if constexpr (TRACE) {
                const long long ta = (long long)__builtin_amdgcn_s_memtime();
                ph[3] += ta - t_top;
                raw_barrier();
                ph[0] += (long long)__builtin_amdgcn_s_memtime() - ta;
            } else {
                raw_barrier();              // batch bi's data and boundary values
            }
        }
        if constexpr (TRACE) {
            if (lane == 0 && tr) tr[bi] = (long long)__builtin_amdgcn_s_memrealtime();
        }
        const double2 *br = reinterpret_cast<const double2 *>(bring + (bi & 1) * 64);
        // issue order = need order: the first pair's boundary values and
        // operands, then the look-ahead pairs, then the remaining boundary
        // values (LDS returns in order, so the first step waits on ~A+1 reads)
        double2 bv[C::PBN];
        const double2 *sc = ring + (bi % C::R) * C::SLOT + lane;
        bv[0] = br[0];
#pragma unroll
        for (int a = 0; a < C::A; a++) rg[0][a] = sc[a * PB];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 1; kk < LK; kk++)
#pragma unroll
            for (int a = 0; a < C::A; a++) rg[kk][a] = sc[a * PB + kk * 64];
#pragma unroll
        for (int kk = 1; kk < C::PBN; kk++) bv[kk] = br[kk];    // broadcast reads
        if constexpr (TRACE) t_top = (long long)__builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        double xv[C::B];
#pragma unroll
        for (int kk = 0; kk < C::PBN; kk++) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int tt = 2 * kk + h;
                const bool sx = FWD ? (h == 0) : (h == 1);     // even step <-> .x
                const double bb = sx ? rg[kk][0].x : rg[kk][0].y;
                const double e1 = sx ? rg[kk][1].x : rg[kk][1].y;
                const double e2 = sx ? rg[kk][2].x : rg[kk][2].y;
                const double old = h ? bv[kk].y : bv[kk].x;
                const double p2 = FM ? 0.0 : e2 * xp;
                // GG_DIV_FMA: the in-line term first, fused, while the line
                // value crosses lanes; b pre-scaled by y = RN(1/d) for U (the
                // coefficients arrive pre-scaled), off the recurrence
                double tf = 0.0;
                if constexpr (FM) {
                    double by = bb;
                    if constexpr (DIV == WD_SFMA) by = bb * (sx ? rg[kk][3].x : rg[kk][3].y);
                    tf = __builtin_fma(-e2, xp, by);
                }
                // 3D: the plane neighbour comes first in the canonical order
                // (|offset| = nx*ny); its term is off the recurrence
                double bz = bb;
                if constexpr (D3) {
                    const double e0 = sx ? rg[kk][C::A2].x : rg[kk][C::A2].y;
                    const double xz = sx ? rg[kk][C::A2 + 1].x : rg[kk][C::A2 + 1].y;
                    bz = bb - e0 * xz;
                }
                const double xs = dpp_shift_old<ctrl>(xp, old);
                if constexpr (SH) {
                    // LDS work of the pair in the cross-lane shift's latency:
                    // the look-ahead reads at the first step, the previous
                    // pair's x staging at the second
                    __builtin_amdgcn_sched_barrier(0);
                    if (h == 0 && kk + LK < C::PBN) {
#pragma unroll
                        for (int a = 0; a < C::A; a++) rg[kk + LK][a] = sc[a * PB + (kk + LK) * 64];
                    }
                    if (h == 1 && kk > 0) {
                        if (FWD) stage(bi & 1, kk - 1, xv[2 * kk - 2], xv[2 * kk - 1]);
                        else stage(bi & 1, kk - 1, xv[2 * kk - 1], xv[2 * kk - 2]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                // the neighbour line's terms oldest first (|offset| = nx, nx-1, ..),
                // then the in-line neighbour (|offset| = 1)
                double acc;
                if constexpr (FM && S == 1) {
                    acc = __builtin_fma(-e1, xs, tf);
                } else if constexpr (FM && S == 2) {
                    // nearest first: in-line (tf), fill nx-1 (xs), line nx (xh1)
                    const double f1 = sx ? rg[kk][C::AE].x : rg[kk][C::AE].y;
                    acc = __builtin_fma(-f1, xs, tf);
                    acc = __builtin_fma(-e1, xh1, acc);
                } else if constexpr (FM) {
                    // in-line, fill nx-2 (xs), fill nx-1 (xh1), line nx (xh2)
                    const double f1 = sx ? rg[kk][C::AE].x : rg[kk][C::AE].y;
                    const double f2 = sx ? rg[kk][C::AE + 1].x : rg[kk][C::AE + 1].y;
                    acc = __builtin_fma(-f2, xs, tf);
                    acc = __builtin_fma(-f1, xh1, acc);
                    acc = __builtin_fma(-e1, xh2, acc);
                } else if constexpr (IL) {
                    acc = bz - p2;
                    acc = acc - e1 * xs;
                } else if constexpr (S == 1) {
                    acc = bz - e1 * xs;
                } else if constexpr (S == 2) {
                    const double f1 = sx ? rg[kk][C::AE].x : rg[kk][C::AE].y;
                    acc = bz - e1 * xh1;
                    acc = acc - f1 * xs;
                } else {
                    const double f1 = sx ? rg[kk][C::AE].x : rg[kk][C::AE].y;
                    const double f2 = sx ? rg[kk][C::AE + 1].x : rg[kk][C::AE + 1].y;
                    acc = bz - e1 * xh2;
                    acc = acc - f1 * xh1;
                    acc = acc - f2 * xs;
                }
                if constexpr (S >= 3) xh2 = xh1;
                if constexpr (S >= 2) xh1 = xs;
                if constexpr (!IL && !FM) acc = acc - p2;
                if constexpr (DIV == WD_HW) {
                    acc = acc / (sx ? rg[kk][3].x : rg[kk][3].y);
                } else if constexpr (DIV == WD_MUL) {
                    acc = acc * (sx ? rg[kk][3].x : rg[kk][3].y);
                } else if constexpr (DIV == WD_RCP) {
                    const double d = sx ? rg[kk][3].x : rg[kk][3].y;
                    const double y = sx ? rg[kk][4].x : rg[kk][4].y;
                    const double q0 = acc * y;
                    const double q1 = __builtin_fma(-__builtin_fma(q0, d, -acc), y, q0);
                    acc = __builtin_fma(-__builtin_fma(q1, d, -acc), y, q1);
                }
                xp = acc;
                xv[tt] = acc;
                if constexpr (TRACE) {      // phase stamps at the first and last step
                    if (tt == 0 || tt == C::B - 1) {
                        const int f = __builtin_amdgcn_readfirstlane(__double2hiint(acc));
                        asm volatile("; use %0" ::"s"(f));
                        const long long now = (long long)__builtin_amdgcn_s_memtime();
                        ph[tt == 0 ? 1 : 2] += now - t_top;
                        t_top = now;
                    }
                }
            }
            // the pair's results go to LDS staging (the writer wave stores them
            // and publishes the edge values), then the pair kWaveLook ahead is
            // read; the scheduling fence keeps it all inside this pair, in the
            // recurrence's latency bubbles
            if (!SH || kk == C::PBN - 1) {
                if (FWD) stage(bi & 1, kk, xv[2 * kk], xv[2 * kk + 1]);
                else stage(bi & 1, kk, xv[2 * kk + 1], xv[2 * kk]);
            }

            if (!SH && kk + LK < C::PBN) {
#pragma unroll
                for (int a = 0; a < C::A; a++) rg[kk + LK][a] = sc[a * PB + (kk + LK) * 64];
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (GG_WAVE_DECOUPLE) {       // the batch's x staging, then the writer's counter
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) __hip_atomic_store(&xdone, seq + bi + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    seq += nbatch;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    raw_barrier();                          // final barrier: the writer drains the last batch
    if (TRACE && lane == 0 && tr) {
        tr[nbatch] = (long long)__builtin_amdgcn_s_memrealtime();
#pragma unroll
        for (int k = 0; k < 4; k++) tr[nbatch + 1 + k] = ph[k];
    }
    };
    if (NC == 1 || wave == 0) compute_wave(std::integral_constant<int, 0>{});
    else if (NC == 2 || wave == 1) compute_wave(std::integral_constant<int, NC >= 2 ? 1 : 0>{});
    else if (NC == 3 || wave == 2) compute_wave(std::integral_constant<int, NC >= 3 ? 2 : 0>{});
    else compute_wave(std::integral_constant<int, NC >= 4 ? 3 : 0>{});
    }   // task loop
}

template <bool FWD, int DIV, bool TRACE, bool D3 = false, int S = 1, bool IL = false>
__global__ __launch_bounds__((WaveCfg<DIV, D3, S>::THREADS)) void k_trsv_wave2d(
    Gate g, int T, int nbands, const double *__restrict__ b, const double *__restrict__ c1,
    const double *__restrict__ c2, const double *__restrict__ dv, const double *__restrict__ rv,
    double *__restrict__ x, unsigned long long *bnd, int *err, long long *trace,
    int nz, long long P2, const double *__restrict__ c0, unsigned long long *prog,
    const double *__restrict__ ce1, const double *__restrict__ ce2, unsigned long long *xw,
    unsigned long long xseq)
{
    trsv_wave2d_body<FWD, DIV, TRACE, D3, S, IL, false>(g, T, nbands, b, c1, c2, dv, rv, x, bnd, err, trace, nz,
                                                        P2, c0, prog, ce1, ce2, FusedSpmv{}, 1, 0, 0, xw, xseq);
}

// forward 2D solve with b = A v computed by the launch's blocks < fs.ns (FusedSpmv)
template <int DIV>
__global__ __launch_bounds__((WaveCfg<DIV>::THREADS)) void k_trsv_wave2d_spmv(
    Gate g, int T, int nbands, const double *__restrict__ c1, const double *__restrict__ c2,
    const double *__restrict__ dv, const double *__restrict__ rv, double *__restrict__ x,
    unsigned long long *bnd, int *err, long long P2, FusedSpmv fs, unsigned long long *xw,
    unsigned long long xseq)
{
    trsv_wave2d_body<true, DIV, false, false, 1, false, true>(g, T, nbands, fs.w, c1, c2, dv, rv, x, bnd, err,
                                                              nullptr, 1, P2, nullptr, nullptr, nullptr, nullptr,
                                                              fs, 1, 0, 0, xw, xseq);
}

// batched 2D solve (the many-RHS solve): zS scenarios, nbands workgroups each
template <bool FWD, int DIV>
__global__ __launch_bounds__((WaveCfg<DIV>::THREADS)) void k_trsv_wave2d_batch(
    Gate g, int T, int nbands, const double *__restrict__ b, const double *__restrict__ c1,
    const double *__restrict__ c2, const double *__restrict__ dv, const double *__restrict__ rv,
    double *__restrict__ x, unsigned long long *bnd, int *err, long long P2, int zS, long long zs, int zmap)
{
    trsv_wave2d_body<FWD, DIV, false, false, 1, false, false, true>(g, T, nbands, b, c1, c2, dv, rv, x, bnd, err,
                                                                    nullptr, 1, P2, nullptr, nullptr, nullptr,
                                                                    nullptr, FusedSpmv{}, zS, zs, zmap);
}

// ================================================ 3D 7-point grids: tile wavefront
// Layout (gg_internal.h Wave2D, tile = true): one wave owns a tile of 8 lines
// x 8 planes, lane l = a + 8 g(c) with the Gray code g(c) = c ^ (c >> 1) for
// plane c = 0..7, and runs point (i, j, k) at step t = i + a + c.  Every term
// of a row is then a recent value of a neighbouring lane: the in-line term the
// lane's own previous step; the line term the previous step one lane down its
// 8-lane half-row (DPP row_shr:1, backward row_shl:1; the half-row's edge lane
// takes the neighbouring tile's value -- as the DPP `old` in half-row 0 of a
// row, by a select in half-row 1); the plane term the previous step's value in
// the predecessor plane's half-row, which differs in one bit of g: one DPP
// row_ror:8 (bit 0), in-place v_permlane16_swap (bit 1) or v_permlane32_swap
// (bit 2) plus selects.  The first plane's half-row takes the neighbouring
// tile's value.  Round 2 skewed planes by two steps so that the plane move ran
// a step ahead, off the recurrence; but the step is issue-bound (≈ 30
// instructions), not chain-bound, and the extra skew cost a K hop 16 steps and
// one more batch of granularity instead of 8: with skew 1 the plane move sits
// on the chain and every hop is 8 steps + one batch.  The dependency chain
// (nx + ny + nz - 2 steps) crosses a workgroup boundary every 8 lines and every
// 8 planes: 26 + 26 hand-offs at 216^3 (round 1: 216 plane hops through HBM).
// Hand-off granules (8 B, value = flag, kSentinel = not ready, re-armed by the
// consumer): per tile and step 16 words, [0, 8) the last plane's half-row for
// tile (J, K +- 1), [8, 16) the eight planes' edge lanes for tile (J +- 1, K).
// The consumer's step t needs the plane and the line granules of step t +- 7
// (same point i, skew a + c).
// Roles as k_trsv_wave2d: wave 0 computes, 1 polls the granules, 2 stores x
// and publishes, 3 streams b, c1, c2 (, d (, RN(1/d))), c0 into the LDS ring.
// Persistent grid, every workgroup co-resident, tiles taken in dependency
// order (host tile_order; the backward solve walks it from the end).
#ifndef GG_TILE_BATCH
#define GG_TILE_BATCH 8
#endif
// 3 slots: 59-70 KiB of LDS, two workgroups per CU -- at the C4 wavefront's
// peak more tiles are ready than there are CUs (C4 L 227 -> 222 us, U 234 ->
// 233 us against 5 slots, profiles/r03/r03_tile_ring.txt)
#ifndef GG_TILE_RING
#define GG_TILE_RING 3
#endif
// boundary wave retries: 0 = one poll at a time, n > 0 = two generations in
// flight, the second issued s_sleep(n) after the first (measured at C4: L/U
// 260-263 / 286-287 us against 246 / 269 -- the extra polls cost more than
// the earlier sight gains)
#ifndef GG_TILE_POLL2
#define GG_TILE_POLL2 0
#endif
template <int DIV>
struct TileCfg {
    static constexpr int A = (DIV == WD_UNIT || DIV == WD_UFMA) ? 4 : DIV == WD_RCP ? 6 : 5;   // WD_MUL / WD_SFMA stream y as d
    static constexpr int AC0 = A - 1;                   // the plane coefficient streams last
    static constexpr int B = GG_TILE_BATCH;
    static constexpr int PBN = B / 2;
    static constexpr int SLOT = A * PBN * 64;           // double2 per ring slot
    static constexpr int NPER = A * PBN;                // DMA instructions per batch
    static constexpr int NG = Wave2D::kTileGran;
    static constexpr int GL = (B * NG + 63) / 64;       // granule loads (stores) per lane per batch
    static constexpr int BND = 2 * PBN * NG;            // boundary values: double2 [2][PBN][NG]
    static constexpr int XST = 2 * PBN * 64;            // x staging: double2 [2][PBN][64]
    static constexpr int RFIT = (150 * 1024 / 16 - BND - XST) / SLOT;
    static constexpr int RVM = 2 + 63 / NPER;
    static constexpr int RING = GG_TILE_RING;
    static constexpr int R = RING < RFIT ? (RING < RVM ? RING : RVM) : (RFIT < RVM ? RFIT : RVM);
    static constexpr int LDS2 = R * SLOT + BND + XST;
    static constexpr int THREADS = 256;
    static_assert(R >= 3 && (R - 2) * NPER <= 63, "ring depth vs vmcnt range");
    static_assert(kTileTAlign % (B * GG_WAVE_POLL) == 0, "steps per tile: whole poll groups of batches");
    static_assert(2 * GL * (GG_WAVE_POLL - 1) <= 63, "boundary wave vmcnt");
    static constexpr int LOOK = kWaveLook < PBN ? kWaveLook : PBN;   // look-ahead pairs
    static_assert(LDS2 * 16 <= 160 * 1024, "LDS budget");
};

__device__ __forceinline__ unsigned bfi(unsigned m, unsigned a, unsigned b) { return (a & m) | (b & ~m); }
__device__ __forceinline__ double bfi64(unsigned m, double a, double b)
{
    return __hiloint2double((int)bfi(m, (unsigned)__double2hiint(a), (unsigned)__double2hiint(b)),
                            (int)bfi(m, (unsigned)__double2loint(a), (unsigned)__double2loint(b)));
}
// per-lane masks of the tile layout (all ones / zero)
struct TileMasks {
    unsigned kb;     // the first plane's half-row: plane term from the neighbouring tile
    unsigned r8;     // plane predecessor one row_ror:8 away (Gray bit 0)
    unsigned p16;    // one v_permlane16_swap away (bit 1); else v_permlane32_swap (bit 2)
    unsigned lfix;   // half-row edge lanes whose line term the DPP shift cannot give
};
// one register as both swap operands exchanges rows in place (checked on the
// GPU, tools/permlane_probe.hip): p16 -> rows (x1, x0, x3, x2), p32 -> (x2, x3,
// x0, x1).  The asm carries the VALU-write -> permlane-read wait states itself.
__device__ __forceinline__ unsigned p16_self(unsigned v)
{
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %0" : "+v"(v));
    return v;
}
__device__ __forceinline__ unsigned p32_self(unsigned v)
{
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %0" : "+v"(v));
    return v;
}
// the plane predecessor's value of x (any lane of the first plane: kb)
__device__ __forceinline__ double plane_move(double x, double kb, const TileMasks &tm)
{
    const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
    const unsigned r8l = (unsigned)__builtin_amdgcn_mov_dpp((int)lo, 0x128, 0xf, 0xf, false);   // row_ror:8
    const unsigned r8h = (unsigned)__builtin_amdgcn_mov_dpp((int)hi, 0x128, 0xf, 0xf, false);
    const unsigned l16 = p16_self(lo), h16 = p16_self(hi), l32 = p32_self(lo), h32 = p32_self(hi);
    const unsigned rlo = bfi(tm.r8, r8l, bfi(tm.p16, l16, l32));
    const unsigned rhi = bfi(tm.r8, r8h, bfi(tm.p16, h16, h32));
    return bfi64(tm.kb, kb, __hiloint2double((int)rhi, (int)rlo));
}

// TRACE (diagnostics, gg_trace_precond): per tile 8 + 5 nbatch words -- compute
// wave's start (barrier 0) and end (realtime, 10 ns), workgroup, boundary-wave
// poll retries and cycles spent retrying, realtime after batch 0 and at the
// loader's first issue; then per batch the compute wave's start, the writer's
// publication, the boundary wave's "all values seen", the loader's "landed"
// and the compute wave's end.
// boundary wave: barrier right after the values are in LDS (1), or after the
// re-arm stores and the next polls are issued (0)
#ifndef GG_TILE_EARLYBAR
#define GG_TILE_EARLYBAR 1
#endif
// writer: publish when the compute wave has staged the batch (1) or at the next
// barrier (0); GG_TILE_WSLEEP: s_sleep between its LDS counter polls
#ifndef GG_TILE_DECOUPLE
#define GG_TILE_DECOUPLE 1
#endif
#ifndef GG_TILE_WSLEEP
#define GG_TILE_WSLEEP 1
#endif

template <bool FWD, int DIV, bool TRACE = false>
__global__ __launch_bounds__(256) void k_trsv_tile3d(
    Gate g, int T, int NJ, int NK, const int *__restrict__ order, const double *__restrict__ b,
    const double *__restrict__ c1, const double *__restrict__ c2, const double *__restrict__ dv,
    const double *__restrict__ rv, const double *__restrict__ c0, double *__restrict__ x,
    unsigned long long *gran, int *err, long long *trace, int dyn)
{
    using C = TileCfg<DIV>;
    constexpr int PB = C::PBN * 64;             // double2 per array per slot
    constexpr int NG = C::NG;
    constexpr int GL = C::GL;
    if (gated(g)) return;
    __shared__ double2 lds[C::LDS2];
    __shared__ int xdone;                       // batches the compute wave has staged (this workgroup)
    double2 *bring = lds + C::R * C::SLOT;      // [2][PBN][32]: [0, 16) plane values, [16, 20) line values
    double2 *xbuf = bring + C::BND;             // [2][PBN][64]
    if (threadIdx.x == 0) xdone = 0;            // read only after the first barrier
    int seq = 0;                                // batches this workgroup has run (uniform)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int np = T / 2;
    const int nbatch = T / C::B;                // T is a multiple of kTileTAlign
    const long long TS = 8 + 5LL * nbatch;      // TRACE words per tile
    const int ntask = NJ * NK;
    const long long tgran = (long long)T * NG;  // granules per tile
    // dummy granules of this workgroup (64 zeros to read, 64 write-only words):
    // a line every boundary wave of the chip polled and re-armed would be a
    // hot spot on one memory channel
    unsigned long long *dummy_ld = gran + (long long)ntask * tgran + (long long)blockIdx.x * 128 + lane;
    unsigned long long *dummy_st = dummy_ld + 64;
    // Tiles are dealt statically (dyn = 0: workgroup w takes every
    // gridDim.x-th tile of the dependency order), which needs the whole grid
    // co-resident -- the grid is sized from the occupancy API, which this pool
    // has seen over-promise.  So the boundary wave's waits are
    // bounded by kResidSpin in that mode: a longer wait sets err bit 3 (8) and
    // the workgroup finishes without waiting (garbage, but the grid drains);
    // the host then reruns with dyn = 1 for the triangle's life: tiles CLAIMED
    // in dependency order from a queue (one agent-scope atomic per tile, issued
    // one tile ahead by the compute wave), where a workgroup claims a tile only
    // while it runs and the smallest unfinished tile's owner has finished every
    // tile it claimed before it -- any grid drains, resident or not.  (The
    // queue is the fallback, not the default: C4 L / U 221.6 / 230.1 us static
    // against 242.7 / 257.3 us claimed, profiles/r04/r04_tile_queue_ab.txt.)
    // q[0] = next tile, q[16] = workgroups finished; the last one re-arms both.
    unsigned long long *q = gran + (long long)ntask * tgran + 128LL * kTileDummyBlocks;
    __shared__ int tq[2];                       // the current and the next claimed tile
    if (threadIdx.x == 0) tq[0] = dyn ? (int)atomicAdd(q, 1ull) : (int)blockIdx.x;
    __syncthreads();
    int kq = 0;                                 // tiles this workgroup has run
    for (int task = tq[0]; task < ntask; task = tq[++kq & 1]) {
    const int band = order[FWD ? task : ntask - 1 - task];
    const int J = band % NJ, K = band / NJ;
    const long long boff = (long long)band * np * 64 + lane;     // double2 units
    if (wave == 3) {
        // ------------------------------------------------ loader wave
        const double2 *src[6] = {reinterpret_cast<const double2 *>(b) + boff,
                                 reinterpret_cast<const double2 *>(c1) + boff,
                                 reinterpret_cast<const double2 *>(c2) + boff,
                                 reinterpret_cast<const double2 *>(dv) + boff,
                                 reinterpret_cast<const double2 *>(rv) + boff, nullptr};
        src[C::AC0] = reinterpret_cast<const double2 *>(c0) + boff;
        if (TRACE && lane == 0) trace[(long long)band * TS + 6] = (long long)__builtin_amdgcn_s_memrealtime();
        wave_loader<FWD, C::R, C::SLOT, C::A, C::PBN>(src, lds, np, nbatch,
                                                      TRACE ? trace + (long long)band * TS + 8 + 3 * nbatch : nullptr);
        raw_barrier();                          // final barrier (the writer drains the last batch)
        continue;
    }
    if (wave == 2) {
        // ------------------------------------------------ writer wave
        // Batch bi's edge values as granules, then x, as soon as the compute
        // wave has staged the batch (LDS counter xdone), not at barrier bi+1:
        // that barrier also waits for batch bi+1's boundary values, and a tile's
        // sources must not hold back what it publishes.
        double2 *X2 = reinterpret_cast<double2 *>(x) + boff;
        unsigned long long *gmine = gran + (long long)band * tgran;
        const bool pub_k = FWD ? (K < NK - 1) : (K > 0);
        const bool pub_j = FWD ? (J < NJ - 1) : (J > 0);
        [[maybe_unused]] bool bad = false;
        raw_barrier();                          // barrier 0
        for (int pb = 0; pb < nbatch; pb++) {
            if constexpr (GG_TILE_DECOUPLE) {
                // wait for the compute wave's counter (its x staging precedes it)
                while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&xdone, __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_WORKGROUP)) <= seq + pb)
                    __builtin_amdgcn_s_sleep(GG_TILE_WSLEEP);
            } else {
                raw_barrier();                  // barrier pb+1
            }
            const double2 *xb = xbuf + (pb & 1) * PB;
#pragma unroll
            for (int m = 0; m < GL; m++) {
                const int e = lane + 64 * m;
                const int tt = e / NG, idx = e - tt * NG;
                if (e < C::B * NG && (idx < 8 ? pub_k : pub_j)) {
                    // the last plane's half-row (forward: plane 7, g = 4; backward:
                    // plane 0, g = 0), or plane c's edge lane (a = 7 / a = 0)
                    const int cq = idx - 8;
                    const int sl = idx < 8 ? (FWD ? 32 + idx : idx) : (FWD ? 7 : 0) + 8 * (cq ^ (cq >> 1));
                    const double v = reinterpret_cast<const double *>(xb + (tt >> 1) * 64 + sl)
                        [FWD ? (tt & 1) : 1 - (tt & 1)];
                    const int t = FWD ? pb * C::B + tt : (T - 1) - (pb * C::B + tt);
                    st_agent(gmine + (long long)t * NG + idx, (unsigned long long)__double_as_longlong(v));
                }
            }
            if (TRACE && lane == 0) trace[(long long)band * TS + 8 + nbatch + pb] = (long long)__builtin_amdgcn_s_memrealtime();
            double2 v[C::PBN];
#pragma unroll
            for (int kk = 0; kk < C::PBN; kk++) v[kk] = xb[kk * 64 + lane];
#pragma unroll
            for (int kk = 0; kk < C::PBN; kk++) {
                const int p = pb * C::PBN + kk;
                X2[(long long)(FWD ? p : np - 1 - p) * 64] = v[kk];
                if constexpr (DIV == WD_RCP) bad |= !rcp_safe(v[kk].x) || !rcp_safe(v[kk].y);
            }
            if constexpr (GG_TILE_DECOUPLE) raw_barrier();   // barrier pb+1 (the last: the task's final one)
        }
        seq += nbatch;
        if constexpr (DIV == WD_RCP) {
            if (__any(bad) && lane == 0) atomicOr(err, 2);
        }
        continue;
    }
    if (wave == 1) {
        // ------------------------------------------------ boundary wave
        // Before barrier bi it places batch bi's boundary values in bring[bi & 1]:
        // entry e = lane + 64 m of the batch is (step tt = e / NG, index e % NG).
        // Polls run kPoll batches deep (GL loads per batch); every lane issues
        // every load and store (unused ones on the dummy granules), which keeps
        // the vmcnt arithmetic exact.
        constexpr int kPoll = GG_WAVE_POLL;
        const bool has_k = FWD ? (K > 0) : (K < NK - 1);
        const bool has_j = FWD ? (J > 0) : (J < NJ - 1);
        unsigned long long *gk = has_k ? gran + (long long)(FWD ? band - NJ : band + NJ) * tgran : gran;
        unsigned long long *gj = has_j ? gran + (long long)(FWD ? band - 1 : band + 1) * tgran : gran;
        auto gaddr = [&](int bj, int m) -> unsigned long long * {
            const int e = lane + 64 * m;
            const int tt = e / NG, idx = e - tt * NG;
            if (e >= C::B * NG || bj >= nbatch) return nullptr;
            const int t = FWD ? bj * C::B + tt : (T - 1) - (bj * C::B + tt);
            const bool pl = idx < 8;
            const int tp = FWD ? t + 7 : t - 7;
            if (!(pl ? has_k : has_j) || tp < 0 || tp >= T) return nullptr;
            return (pl ? gk : gj) + (long long)tp * NG + idx;
        };
        auto paddr = [&](int bj, int m) {
            unsigned long long *a = gaddr(bj, m);
            return a ? a : dummy_ld;
        };
        unsigned long long v[kPoll][GL];
#pragma unroll
        for (int u = 0; u < kPoll; u++) {
            if (u > 0) {
#pragma unroll
                for (int m = 0; m < GL; m++) st_agent(dummy_st, kSentinel);
            }
#pragma unroll
            for (int m = 0; m < GL; m++) v[u][m] = ld_agent(paddr(u, m));
        }
        bool dead = false;
        long long bw_spins = 0, bw_cyc = 0;     // TRACE
        for (int bi0 = 0; bi0 < nbatch; bi0 += kPoll) {     // nbatch is a multiple of kPoll
#pragma unroll
            for (int u = 0; u < kPoll; u++) {
                const int bi = bi0 + u;
                // this batch's polls done: after them come kPoll-1 batches of
                // GL re-arm stores and GL loads
                __builtin_amdgcn_s_waitcnt(vm_wait(2 * GL * (kPoll - 1)));
                int spins = 0;
                const long long tw = TRACE ? (long long)__builtin_amdgcn_s_memtime() : 0;
                auto ready = [&]() {
                    bool r = true;
#pragma unroll
                    for (int m = 0; m < GL; m++) r = r && v[u][m] != kSentinel;
                    return r;
                };
                if constexpr (GG_TILE_POLL2) {
                    // not ready: two poll generations in flight, staggered, so a
                    // value that lands is seen within about half a round trip
                    // (every load completes in order: vm_wait(GL) = the older
                    // generation is back)
                    if (!__all(ready())) {
                        unsigned long long pa[GL], pb2[GL];
#pragma unroll
                        for (int m = 0; m < GL; m++) pa[m] = ld_agent(paddr(bi, m));
                        __builtin_amdgcn_s_sleep(GG_TILE_POLL2);
#pragma unroll
                        for (int m = 0; m < GL; m++) pb2[m] = ld_agent(paddr(bi, m));
                        auto rdy = [&](const unsigned long long *q) {
                            bool r = true;
#pragma unroll
                            for (int m = 0; m < GL; m++) r = r && q[m] != kSentinel;
                            return r;
                        };
                        while (true) {
                            __builtin_amdgcn_s_waitcnt(vm_wait(GL));
                            if (dead || __all(rdy(pa))) {
#pragma unroll
                                for (int m = 0; m < GL; m++) v[u][m] = pa[m];
                                break;
                            }
#pragma unroll
                            for (int m = 0; m < GL; m++) pa[m] = ld_agent(paddr(bi, m));
                            __builtin_amdgcn_s_waitcnt(vm_wait(GL));
                            if (__all(rdy(pb2))) {
#pragma unroll
                                for (int m = 0; m < GL; m++) v[u][m] = pb2[m];
                                break;
                            }
#pragma unroll
                            for (int m = 0; m < GL; m++) pb2[m] = ld_agent(paddr(bi, m));
                            spins += 2;
                            if (spins > kSpinLimit) {
                                dead = true;
                                if (lane == 0) atomicOr(err, 1);
                            }
                        }
                        __builtin_amdgcn_s_waitcnt(vm_wait(0));   // the other generation
                    }
                } else {
                    while (!dead && !__all(ready())) {
                        __builtin_amdgcn_s_sleep(1);
#pragma unroll
                        for (int m = 0; m < GL; m++) v[u][m] = ld_agent(paddr(bi, m));
                        if (++spins > (dyn ? kSpinLimit : kResidSpin)) {
                            dead = true;
                            if (lane == 0) atomicOr(err, dyn ? 1 : 8);   // 8: static grid not resident
                        }
                        __builtin_amdgcn_s_waitcnt(vm_wait(0));
                    }
                }
                if constexpr (TRACE) {
                    bw_spins += spins;
                    if (spins) bw_cyc += (long long)__builtin_amdgcn_s_memtime() - tw;
                    if (lane == 0) trace[(long long)band * TS + 8 + 2 * nbatch + bi] = (long long)__builtin_amdgcn_s_memrealtime();
                }
                double *bd = reinterpret_cast<double *>(bring + (bi & 1) * (C::PBN * NG));
#pragma unroll
                for (int m = 0; m < GL; m++) {
                    const int e = lane + 64 * m;
                    const int tt = e / NG, idx = e - tt * NG;
                    if (e < C::B * NG) bd[((tt >> 1) * NG + idx) * 2 + (tt & 1)] = __longlong_as_double((long long)v[u][m]);
                }
                if constexpr (GG_TILE_EARLYBAR) {
                    // hand the values over first, then re-arm and poll ahead
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    raw_barrier();
                }
#pragma unroll
                for (int m = 0; m < GL; m++) {
                    unsigned long long *ga = gaddr(bi, m);
                    st_agent(ga ? ga : dummy_st, kSentinel);     // re-arm for the next launch
                }
#pragma unroll
                for (int m = 0; m < GL; m++) v[u][m] = ld_agent(paddr(bi + kPoll, m));
                if constexpr (!GG_TILE_EARLYBAR) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    raw_barrier();
                }
            }
        }
        raw_barrier();                      // final barrier (the writer drains the last batch)
        if (TRACE && lane == 0) {
            trace[(long long)band * TS + 3] = bw_spins;
            trace[(long long)band * TS + 4] = bw_cyc;
        }
        continue;
    }

    // ---------------------------------------------------- compute wave
    constexpr int ctrl = FWD ? 0x111 : 0x101;   // row_shr:1 / row_shl:1
    const int la = lane & 7, hr = lane >> 3;
    const int cp = hr ^ (hr >> 1) ^ (hr >> 2);  // this lane's plane (inverse Gray code)
    const int cs = FWD ? cp : cp + 1;           // the plane whose predecessor move applies
    const TileMasks tm{(FWD ? cp == 0 : cp == 7) ? ~0u : 0u, (cs & 1) ? ~0u : 0u, (cs & 3) == 2 ? ~0u : 0u,
                       (lane & 15) == (FWD ? 8 : 7) ? ~0u : 0u};
    double xp = 0.0;                        // this lane's value of the previous step
    double2 rg[C::PBN][C::A];
    raw_barrier();                          // barrier 0: batch 0 is in LDS
    // the next tile, claimed now (its latency hides in this tile's batches)
    // and handed to every wave through LDS before the task's final barrier
    int next_task = 0;
    if (lane == 0) next_task = dyn ? (int)atomicAdd(q, 1ull) : task + (int)gridDim.x;
    if (TRACE && lane == 0) {
        trace[(long long)band * TS + 0] = (long long)__builtin_amdgcn_s_memrealtime();
        trace[(long long)band * TS + 2] = blockIdx.x;
    }
    for (int bi = 0; bi < nbatch; bi++) {
        // the first step's plane neighbour (the previous step) is moved before
        // the barrier; only the first plane's row waits for the boundary value
        const double xzp = plane_move(xp, 0.0, tm);
        if (bi > 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // x staging of batch bi-1 written
            raw_barrier();                  // batch bi's data and boundary values
            if (TRACE && bi == 1 && lane == 0) trace[(long long)band * TS + 5] = (long long)__builtin_amdgcn_s_memrealtime();
        }
        if (TRACE && lane == 0) trace[(long long)band * TS + 8 + bi] = (long long)__builtin_amdgcn_s_memrealtime();
        const double2 *br = bring + (bi & 1) * (C::PBN * NG);
        const double2 *sc = lds + (bi % C::R) * C::SLOT + lane;
        double2 bk[C::PBN], bj[C::PBN];     // plane / line boundary values of each step pair
        bk[0] = br[la];
        bj[0] = br[8 + cp];
#pragma unroll
        for (int a = 0; a < C::A; a++) rg[0][a] = sc[a * PB];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 1; kk < C::LOOK; kk++)
#pragma unroll
            for (int a = 0; a < C::A; a++) rg[kk][a] = sc[a * PB + kk * 64];
#pragma unroll
        for (int kk = 1; kk < C::PBN; kk++) {
            bk[kk] = br[kk * NG + la];
            bj[kk] = br[kk * NG + 8 + cp];
        }
        __builtin_amdgcn_sched_barrier(0);
        double xv[C::B];
        // the plane neighbour's value for the batch's first step
        const double xz0 = bfi64(tm.kb, bk[0].x, xzp);
#pragma unroll
        for (int kk = 0; kk < C::PBN; kk++) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int tt = 2 * kk + h;
                const bool sx = FWD ? (h == 0) : (h == 1);     // even storage step <-> .x
                const double bb = sx ? rg[kk][0].x : rg[kk][0].y;
                const double e1 = sx ? rg[kk][1].x : rg[kk][1].y;
                const double e2 = sx ? rg[kk][2].x : rg[kk][2].y;
                const double e0 = sx ? rg[kk][C::AC0].x : rg[kk][C::AC0].y;
                const double oj = h ? bj[kk].y : bj[kk].x;      // boundary entries by sweep step
                // the plane neighbour: the predecessor plane's value of the previous step
                const double xz = tt == 0 ? xz0 : plane_move(xp, h ? bk[kk].y : bk[kk].x, tm);
                const double p2 = (DIV == WD_UFMA || DIV == WD_SFMA) ? 0.0 : e2 * xp;
                const double xs = bfi64(tm.lfix, oj, dpp_shift_old<ctrl>(xp, oj));
                if constexpr (kWaveShadow) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (h == 0 && kk + C::LOOK < C::PBN) {
#pragma unroll
                        for (int a = 0; a < C::A; a++) rg[kk + C::LOOK][a] = sc[a * PB + (kk + C::LOOK) * 64];
                    }
                    if (h == 1 && kk > 0) {
                        xbuf[(bi & 1) * PB + (kk - 1) * 64 + lane] =
                            FWD ? make_double2(xv[2 * kk - 2], xv[2 * kk - 1])
                                : make_double2(xv[2 * kk - 1], xv[2 * kk - 2]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                // canonical order: plane term, line term, in-line term;
                // GG_DIV_FMA: nearest first, fused (in-line, line, plane: the
                // order the operands arrive in), b pre-scaled for U
                double acc;
                if constexpr (DIV == WD_UFMA || DIV == WD_SFMA) {
                    double by = bb;
                    if constexpr (DIV == WD_SFMA) by = bb * (sx ? rg[kk][3].x : rg[kk][3].y);
                    acc = __builtin_fma(-e2, xp, by);
                    acc = __builtin_fma(-e1, xs, acc);
                    acc = __builtin_fma(-e0, xz, acc);
                } else {
                    acc = bb - e0 * xz;
                    acc = acc - e1 * xs;
                    acc = acc - p2;
                }
                if constexpr (DIV == WD_HW) {
                    acc = acc / (sx ? rg[kk][3].x : rg[kk][3].y);
                } else if constexpr (DIV == WD_MUL) {
                    acc = acc * (sx ? rg[kk][3].x : rg[kk][3].y);
                } else if constexpr (DIV == WD_RCP) {
                    const double d = sx ? rg[kk][3].x : rg[kk][3].y;
                    const double y = sx ? rg[kk][4].x : rg[kk][4].y;
                    const double q0 = acc * y;
                    const double q1 = __builtin_fma(-__builtin_fma(q0, d, -acc), y, q0);
                    acc = __builtin_fma(-__builtin_fma(q1, d, -acc), y, q1);
                }
                xp = acc;
                xv[tt] = acc;
            }
            if (!kWaveShadow || kk == C::PBN - 1)
                xbuf[(bi & 1) * PB + kk * 64 + lane] =
                    FWD ? make_double2(xv[2 * kk], xv[2 * kk + 1]) : make_double2(xv[2 * kk + 1], xv[2 * kk]);
            if (!kWaveShadow && kk + C::LOOK < C::PBN) {
#pragma unroll
                for (int a = 0; a < C::A; a++) rg[kk + C::LOOK][a] = sc[a * PB + (kk + C::LOOK) * 64];
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // the batch's x staging, then the writer's counter
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (TRACE && lane == 0) trace[(long long)band * TS + 8 + 4 * nbatch + bi] = (long long)__builtin_amdgcn_s_memrealtime();
        if (GG_TILE_DECOUPLE && lane == 0)
            __hip_atomic_store(&xdone, seq + bi + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    seq += nbatch;
    if (lane == 0) tq[(kq + 1) & 1] = next_task;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    raw_barrier();                          // final barrier: the writer drains the last batch
    if (TRACE && lane == 0) trace[(long long)band * TS + 1] = (long long)__builtin_amdgcn_s_memrealtime();
    }   // task loop
    // every claim of this workgroup has returned: count it out; the last
    // workgroup re-arms the queue (the next launch follows a kernel boundary)
    if (dyn && threadIdx.x == 0) {
        if (atomicAdd(q + 16, 1ull) == (unsigned long long)gridDim.x - 1) {
            st_agent(q, 0ull);
            st_agent(q + 16, 0ull);
        }
    }
}

}  // namespace

template <bool FWD, int DIV>
int wave3d_max_blocks()
{
    static int cached = -1;
    if (cached < 0)
        cached = std::max(1, resident_blocks(k_trsv_wave2d<FWD, DIV, false, true>, WaveCfg<DIV, true>::THREADS));
    return cached;
}

template <bool FWD, int DIV>
int tile3d_max_blocks()
{
    static int cached = -1;
    if (cached < 0) cached = std::max(1, resident_blocks(k_trsv_tile3d<FWD, DIV>, TileCfg<DIV>::THREADS));
    return cached;
}

int tile_batch_steps() { return GG_TILE_BATCH; }

// tests: GG_TILE_GRID = workgroups of the tile solve (beyond what can be
// resident: the task queue must still drain it)
// the tile solve's mode: static (0) unless the triangle fell back to the
// queue (1); GG_TILE_QUEUE=1 forces the queue (tests, A/B)
static int tile_dyn(const DevTri &T)
{
    const char *e = std::getenv("GG_TILE_QUEUE");
    return (T.tile_queue || (e && e[0] == '1')) ? 1 : 0;
}
static int tile_grid_override(int g)
{
    const char *e = std::getenv("GG_TILE_GRID");
    return e && atoi(e) > 0 ? atoi(e) : g;
}

int wave_band_candidate(int nbands, int ng, int k)
{
    if (nbands < 1 || ng < 1 || ng > kWaveCand || k < 0 || k >= nbands) return -1;
    return wave_candidate(nbands, ng, k);
}
int wave_band_candidates() { return kWaveCand; }

int wave_batch_steps(int div, bool d3, int skew)
{
    // WD_MUL streams as many arrays as WD_HW (y in d's place): the same batches
    const bool hw = div == WD_HW || div == WD_MUL;
    if (d3) return div == WD_UNIT ? WaveCfg<WD_UNIT, true>::B : hw ? WaveCfg<WD_HW, true>::B
                                                                   : WaveCfg<WD_RCP, true>::B;
    if (skew == 2)
        return div == WD_UNIT ? WaveCfg<WD_UNIT, false, 2>::B : hw ? WaveCfg<WD_HW, false, 2>::B
                                                                   : WaveCfg<WD_RCP, false, 2>::B;
    if (skew == 3)
        return div == WD_UNIT ? WaveCfg<WD_UNIT, false, 3>::B : hw ? WaveCfg<WD_HW, false, 3>::B
                                                                   : WaveCfg<WD_RCP, false, 3>::B;
    if (div == WD_UFMA) return WaveCfg<WD_UFMA>::B;
    if (div == WD_SFMA) return WaveCfg<WD_SFMA>::B;
    return div == WD_UNIT ? WaveCfg<WD_UNIT>::B : hw ? WaveCfg<WD_HW>::B : WaveCfg<WD_RCP>::B;
}

bool fused_spmv_ok(const DevTri &T, const DevCsr &A)
{
    const Wave2D &w = T.wl;
    return T.kind == DevTri::WAVE2D && T.lower && !T.tail && w.ok && !w.tile && w.nz == 1 && w.skew == 1 && !T.trace &&
           (T.eff_div() == WD_UFMA || T.eff_div() == WD_SFMA) && A.sell && w.T % kFsGroup == 0 &&
           (long long)A.nslice >= (long long)w.nbands * w.T && (long long)A.n >= (long long)w.nbands * w.T * 64;
}

void launch_trsv_spmv(Gate g, DevTri &T, const DevCsr &A, const double *v, double *w, double *x, int *err,
                      hipStream_t st, const double *ydiv, const double *xdiv)
{
    const Wave2D &wl = T.wl;
    const size_t nflag = (size_t)wl.nbands * (wl.T / kFsGroup);
    if (T.fcnt.n < nflag) {
        T.fcnt.alloc(nflag);
        GG_HIP(hipMemsetAsync(T.fcnt.p, 0, nflag * sizeof(unsigned long long), st));
    }
    // every CU the bands leave free computes b (the SpMV blocks wait on nothing)
    static const int cus = device_cus();
    // (of a band's wave_deal candidate workgroups all but one exit at once, but
    // the dispatcher deals them all: GG_WAVE_FS_SPARE CUs per band stay free of
    // SpMV blocks, so that the XCD of a group has room for its bands)
    const int deal = wave_deal_fs(T.eff_div());
    const int ns = std::max(64, cus - wl.nbands * (deal > 1 ? GG_WAVE_FS_SPARE : 1));
    const int nwg = wl.nbands * deal + ns;
    const unsigned long long xseq = ++T.xseq;
    FusedSpmv fs;
    fs.sptr = A.sptr.p;
    fs.sci = A.sci.p;
    fs.sv = A.sv.p;
    fs.v = v;
    fs.w = w;
    fs.cnt = T.fcnt.p;
    fs.ydiv = ydiv;
    fs.xdiv = xdiv;
    fs.n = A.n;
    fs.ns = ns;
    if (T.eff_div() == WD_UFMA)
        k_trsv_wave2d_spmv<WD_UFMA><<<nwg, WaveCfg<WD_UFMA>::THREADS, 0, st>>>(
            g, wl.T, wl.nbands, T.c1.p, T.c2.p, nullptr, nullptr, x, T.bnd.p, err, wl.P2, fs, T.xw, xseq);
    else   // the split engine's non-unit L, coefficients and b pre-scaled by RN(1/d)
        k_trsv_wave2d_spmv<WD_SFMA><<<nwg, WaveCfg<WD_SFMA>::THREADS, 0, st>>>(
            g, wl.T, wl.nbands, T.c1s.p, T.c2s.p, T.rw.p, nullptr, x, T.bnd.p, err, wl.P2, fs, T.xw, xseq);
}

void launch_trsv_one(Gate g, DevTri &T, const double *b, double *x, int *err, hipStream_t st)
{
    if (T.kind == DevTri::LEVEL) {
        launch_trsv_levels(g, T, b, x, err, st);
    } else if (T.kind == DevTri::WAVE2D) {
        const Wave2D &w = T.wl;
        const int div = T.eff_div();
        // WD_MUL / WD_SFMA stream y = RN(1/d) in d's place
        const double *dv = (div == WD_UNIT || div == WD_UFMA) ? nullptr
                         : (div == WD_MUL || div == WD_SFMA) ? T.rw.p : T.dw.p;
        const double *rv = div == WD_RCP ? T.rw.p : nullptr;
        const unsigned long long xseq = ++T.xseq;       // the launch's number (the bands' XCD words)
        if ((div == WD_UFMA || div == WD_SFMA) && !w.tile) {
            // GG_DIV_FMA on a 2D grid (build_tri admits unskewed ones in canonical order)
            dim3 grid(w.nbands * wave_deal(T.lower));
            const double *k1 = div == WD_SFMA ? T.c1s.p : T.c1.p, *k2 = div == WD_SFMA ? T.c2s.p : T.c2.p;
            if (w.skew > 1) {
                // ILU(k) grids (skewed lanes): the fills pre-scaled with U's coefficients
                const double *f1 = div == WD_SFMA ? T.ce1s.p : T.ce1.p, *f2 = div == WD_SFMA ? T.ce2s.p : T.ce2.p;
#define GG_FMA_SKEW_LAUNCH(FWD, DIV, S)                                                            \
    k_trsv_wave2d<FWD, DIV, false, false, S, false><<<grid, WaveCfg<DIV, false, S>::THREADS, 0, st>>>( \
        g, w.T, w.nbands, b, k1, k2, dv, rv, x, T.bnd.p, err, nullptr, 1, w.P2, nullptr, nullptr, f1, f2, T.xw, xseq)
                if (T.lower && div == WD_UFMA) {
                    if (w.skew == 2) GG_FMA_SKEW_LAUNCH(true, WD_UFMA, 2);
                    else GG_FMA_SKEW_LAUNCH(true, WD_UFMA, 3);
                } else if (!T.lower && div == WD_SFMA) {
                    if (w.skew == 2) GG_FMA_SKEW_LAUNCH(false, WD_SFMA, 2);
                    else GG_FMA_SKEW_LAUNCH(false, WD_SFMA, 3);
                } else if (T.lower && div == WD_SFMA) {
                    if (w.skew == 2) GG_FMA_SKEW_LAUNCH(true, WD_SFMA, 2);
                    else GG_FMA_SKEW_LAUNCH(true, WD_SFMA, 3);
                } else {
                    std::abort();   // build_tri: no unit upper triangle
                }
#undef GG_FMA_SKEW_LAUNCH
                return;
            }
#define GG_FMA_LAUNCH(FWD, DIV, TR)                                                                \
    k_trsv_wave2d<FWD, DIV, TR><<<grid, WaveCfg<DIV>::THREADS, 0, st>>>(                           \
        g, w.T, w.nbands, b, k1, k2, dv, rv, x, T.bnd.p, err, T.trace, 1, w.P2, nullptr, nullptr,   \
        nullptr, nullptr, T.xw, xseq)
            // (T.il needs no instantiation of its own: the fused rows take the
            // in-line term first in either canonical order)
            if (T.lower && div == WD_UFMA) {
                if (T.trace) GG_FMA_LAUNCH(true, WD_UFMA, true);
                else GG_FMA_LAUNCH(true, WD_UFMA, false);
            } else if (!T.lower && div == WD_SFMA) {
                if (T.trace) GG_FMA_LAUNCH(false, WD_SFMA, true);
                else GG_FMA_LAUNCH(false, WD_SFMA, false);
            } else if (T.lower && div == WD_SFMA) {
                GG_FMA_LAUNCH(true, WD_SFMA, false);      // the split engine's non-unit L
            } else
#undef GG_FMA_LAUNCH
                std::abort();   // build_tri: no unit upper triangle
        } else if (w.tile) {
            // 3D tiles: persistent, every workgroup co-resident (tiles wait on tiles)
            const int ntask = w.nbands;
            const bool sc = div == WD_SFMA;     // GG_DIV_FMA's U: coefficients pre-scaled by RN(1/d)
            const double *k1 = sc ? T.c1s.p : T.c1.p, *k2 = sc ? T.c2s.p : T.c2.p, *k0 = sc ? T.c0s.p : T.c0.p;
#define GG_TILE_LAUNCH(FWD, DIV)                                                                   \
    do {                                                                                           \
        const int grid = std::min(std::min(ntask, tile_grid_override(tile3d_max_blocks<FWD, DIV>())), \
                                  kTileDummyBlocks);                                                     \
        if (T.trace)                                                                               \
            k_trsv_tile3d<FWD, DIV, true><<<grid, TileCfg<DIV>::THREADS, 0, st>>>(                 \
                g, w.T, w.NJ, w.NK, T.order.p, b, k1, k2, dv, rv, k0, x, T.bnd.p, err,              \
                T.trace, tile_dyn(T));                                                             \
        else                                                                                       \
            k_trsv_tile3d<FWD, DIV><<<grid, TileCfg<DIV>::THREADS, 0, st>>>(                       \
                g, w.T, w.NJ, w.NK, T.order.p, b, k1, k2, dv, rv, k0, x, T.bnd.p, err,              \
                nullptr, tile_dyn(T));                                                             \
    } while (0)
            if (div == WD_UFMA || div == WD_SFMA) {
                // GG_DIV_FMA (build_tri admits the unit L and a non-unit U)
                if (T.lower && div == WD_UFMA) GG_TILE_LAUNCH(true, WD_UFMA);
                else if (!T.lower && div == WD_SFMA) GG_TILE_LAUNCH(false, WD_SFMA);
                else std::abort();
            } else if (T.lower) {
                if (div == WD_UNIT) GG_TILE_LAUNCH(true, WD_UNIT);
                else if (div == WD_HW) GG_TILE_LAUNCH(true, WD_HW);
                else if (div == WD_MUL) GG_TILE_LAUNCH(true, WD_MUL);
                else GG_TILE_LAUNCH(true, WD_RCP);
            } else {
                if (div == WD_UNIT) GG_TILE_LAUNCH(false, WD_UNIT);
                else if (div == WD_HW) GG_TILE_LAUNCH(false, WD_HW);
                else if (div == WD_MUL) GG_TILE_LAUNCH(false, WD_MUL);
                else GG_TILE_LAUNCH(false, WD_RCP);
            }
#undef GG_TILE_LAUNCH
        } else if (w.nz == 1) {
            dim3 grid(w.nbands * wave_deal(T.lower));
#define GG_WAVE_LAUNCH_S(FWD, DIV, S, IL)                                                          \
    k_trsv_wave2d<FWD, DIV, false, false, S, IL><<<grid, WaveCfg<DIV, false, S>::THREADS, 0, st>>>( \
        g, w.T, w.nbands, b, T.c1.p, T.c2.p, dv, rv, x, T.bnd.p, err, nullptr, 1, w.P2, nullptr,   \
        nullptr, T.ce1.p, T.ce2.p, T.xw, xseq)
#define GG_WAVE_LAUNCH(FWD, DIV)                                                                   \
    do {                                                                                           \
        if (T.trace && w.skew == 1 && !T.il)                                                       \
            k_trsv_wave2d<FWD, DIV, true><<<grid, WaveCfg<DIV>::THREADS, 0, st>>>(                 \
                g, w.T, w.nbands, b, T.c1.p, T.c2.p, dv, rv, x, T.bnd.p, err, T.trace, 1, w.P2,     \
                nullptr, nullptr, nullptr, nullptr, T.xw, xseq);                                               \
        else if (T.il)                                                                             \
            GG_WAVE_LAUNCH_S(FWD, DIV, 1, true);                                                   \
        else if (w.skew == 1)                                                                      \
            GG_WAVE_LAUNCH_S(FWD, DIV, 1, false);                                                  \
        else if (w.skew == 2)                                                                      \
            GG_WAVE_LAUNCH_S(FWD, DIV, 2, false);                                                  \
        else                                                                                       \
            GG_WAVE_LAUNCH_S(FWD, DIV, 3, false);                                                  \
    } while (0)
            if (T.lower) {
                if (div == WD_UNIT) GG_WAVE_LAUNCH(true, WD_UNIT);
                else if (div == WD_HW) GG_WAVE_LAUNCH(true, WD_HW);
                else if (div == WD_MUL) GG_WAVE_LAUNCH(true, WD_MUL);
                else GG_WAVE_LAUNCH(true, WD_RCP);
            } else {
                if (div == WD_UNIT) GG_WAVE_LAUNCH(false, WD_UNIT);
                else if (div == WD_HW) GG_WAVE_LAUNCH(false, WD_HW);
                else if (div == WD_MUL) GG_WAVE_LAUNCH(false, WD_MUL);
                else GG_WAVE_LAUNCH(false, WD_RCP);
            }
#undef GG_WAVE_LAUNCH
#undef GG_WAVE_LAUNCH_S
        } else {
            // 3D: persistent, every workgroup co-resident (tasks wait on tasks)
            const int ntask = w.nz * w.nbands;
#define GG_WAVE_LAUNCH3(FWD, DIV)                                                                  \
    do {                                                                                           \
        const int grid = std::min(std::min(ntask, wave3d_max_blocks<FWD, DIV>()), kTileDummyBlocks); \
        k_trsv_wave2d<FWD, DIV, false, true><<<grid, WaveCfg<DIV, true>::THREADS, 0, st>>>(        \
            g, w.T, w.nbands, b, T.c1.p, T.c2.p, dv, rv, x, T.bnd.p, err, nullptr, w.nz, w.P2,      \
            T.c0.p, T.prog.p, nullptr, nullptr, nullptr, 0ull);                                                   \
    } while (0)
            if (T.lower) {
                if (div == WD_UNIT) GG_WAVE_LAUNCH3(true, WD_UNIT);
                else if (div == WD_HW) GG_WAVE_LAUNCH3(true, WD_HW);
                else if (div == WD_MUL) GG_WAVE_LAUNCH3(true, WD_MUL);
                else GG_WAVE_LAUNCH3(true, WD_RCP);
            } else {
                if (div == WD_UNIT) GG_WAVE_LAUNCH3(false, WD_UNIT);
                else if (div == WD_HW) GG_WAVE_LAUNCH3(false, WD_HW);
                else if (div == WD_MUL) GG_WAVE_LAUNCH3(false, WD_MUL);
                else GG_WAVE_LAUNCH3(false, WD_RCP);
            }
#undef GG_WAVE_LAUNCH3
        }
    }
}

bool trsv_batchable(const DevTri &T)
{
    const Wave2D &w = T.wl;
    if (T.kind != DevTri::WAVE2D || T.tail || !w.ok || w.tile || w.nz != 1 || w.skew != 1 || T.il || T.trace)
        return false;
    const int e = T.eff_div();
    return T.lower ? (e == WD_UNIT || e == WD_UFMA) : (e == WD_HW || e == WD_RCP || e == WD_MUL || e == WD_SFMA);
}
// the batched wavefront's workgroup map (trsv_wave2d_body's zmap), default 1:
// band b of every scenario on one XCD, so the scenarios share its coefficient
// streams in the L2 -- C5 with 8 scenarios (one box, rocprofv3 FETCH_SIZE,
// profiles/r06/c5_batch_pmc.txt): U 236 -> 83 MB, L 177 -> 75 MB per launch,
// 10,500 -> 10,751 it/s; 0: a scenario's bands on one XCD
int batch_zmap()
{
    static const int z = [] {
        const char *e = std::getenv("GG_BATCH_ZMAP");
        return e ? std::atoi(e) : 1;
    }();
    return z;
}
void launch_trsv_b(Gate g, DevTri &T, const double *b, double *x, unsigned long long *bnd, int *err, int nsc,
                   long long zs, hipStream_t st)
{
    GG_REQUIRE(trsv_batchable(T), GG_EINVAL, "batched triangular solve: 2D wavefront, canonical order only");
    const Wave2D &w = T.wl;
    const int e = T.eff_div();
    const int zmap = batch_zmap();
    const dim3 grid(w.nbands * nsc);
    const double *k1 = e == WD_SFMA ? T.c1s.p : T.c1.p, *k2 = e == WD_SFMA ? T.c2s.p : T.c2.p;
    const double *dv = (e == WD_UNIT || e == WD_UFMA) ? nullptr : (e == WD_MUL || e == WD_SFMA) ? T.rw.p : T.dw.p;
    const double *rv = e == WD_RCP ? T.rw.p : nullptr;
    static const bool s1single = [] {
        const char *e = std::getenv("GG_BATCH_S1_SINGLE");     // diagnostics: one scenario on the single kernel
        return e && e[0] == '1';
    }();
    if (nsc == 1 && s1single) {
        DevTri &T2 = T;
        unsigned long long *keep = T2.bnd.p;
        T2.bnd.p = bnd;
        launch_trsv(g, T2, b, x, err, st);
        T2.bnd.p = keep;
        return;
    }
#define GG_BT(FWD, DIV)                                                                                     \
    k_trsv_wave2d_batch<FWD, DIV><<<grid, WaveCfg<DIV>::THREADS, 0, st>>>(g, w.T, w.nbands, b, k1, k2, dv, rv, \
                                                                          x, bnd, err, w.P2, nsc, zs, zmap)
    if (T.lower) {
        if (e == WD_UFMA) GG_BT(true, WD_UFMA);
        else GG_BT(true, WD_UNIT);
    } else {
        if (e == WD_SFMA) GG_BT(false, WD_SFMA);
        else if (e == WD_MUL) GG_BT(false, WD_MUL);
        else if (e == WD_RCP) GG_BT(false, WD_RCP);
        else GG_BT(false, WD_HW);
    }
#undef GG_BT
}
long long trsv_b_granules(const DevTri &T)
{
    // hand-off granules, then per band workgroup 64 zero + 64 write-only dummies, + 64
    return T.wl.ngran() + 128LL * T.wl.nbands + 64;
}

}  // namespace gg
