// kernels/device.h -- device helpers shared by the hand-written gfx950 (CDNA4) kernels for the GMRES hot path
// (kernels.hip and the family files beside this header).
//
// Arithmetic order: every kernel that has a serial counterpart in the
// reference (SpMV row sums, triangular-solve rows, AXPY, Update) evaluates
// the same expression in the same order with contraction disabled
// (-ffp-contract=off), so it is bit-identical to the fp64 restatement.  Only
// the dot products / norms (wave-shuffle trees) round differently.
//
// Wave = 64 lanes; vector kernels use 256-thread blocks and 16-B (double2)
// loads; every reduction is a fixed tree (deterministic, no atomics).
#pragma once

#include <hip/hip_runtime.h>
#include <type_traits>

#include "kernels.h"

namespace gg {

namespace {

__device__ __forceinline__ bool gated(const Gate &g)
{
    if (g.done && (*g.done & g.mask)) return true;
    if (g.nit && g.i >= *g.nit) return true;
    return false;
}

// Batched launches (kernels.h, the many-RHS solve): scenario sc's copy of a
// per-scenario buffer (vectors, partials, H, the control block, hand-off
// granules -- one arena per scenario) lies sc * zs bytes after scenario 0's.
// zs = 0: the single-scenario launch, every pointer as given.
// (char-pointer arithmetic, not an integer round trip: the compiler keeps the
// global address space -- global_* instead of flat_* accesses, which the
// wavefront kernel's writer could not afford)
template <class T>
__device__ __forceinline__ T *zp(T *p, long long zs, int sc)
{
    using C = typename std::conditional<std::is_const<T>::value, const char, char>::type;
    return reinterpret_cast<T *>(reinterpret_cast<C *>(p) + (long long)sc * zs);
}
__device__ __forceinline__ bool gated_z(const Gate &g, long long zs, int sc)
{
    Gate h = g;
    if (g.done) h.done = zp(g.done, zs, sc);
    if (g.nit) h.nit = zp(g.nit, zs, sc);
    return gated(h);
}

// ---- reductions -------------------------------------------------------------
// The xor butterfly v += v[lane ^ o], o = 32, 16, .., 1 (every lane ends with
// the same sum).  After the steps above o, v depends only on the lane bits
// below 2o, so any lane that agrees with lane ^ o on the bits below o and
// differs in bit o holds v[lane ^ o]: in-place v_permlane32 / 16 swaps (o =
// 32, 16) and DPP row_ror:o within rows of 16 (o = 8 .. 1; adding o mod 16
// flips bit o and keeps the lower bits).  The same operands in the same order
// as the ds_bpermute form (__shfl_xor), so the same bits, at VALU latency
// instead of six LDS round trips.  GG_WAVE_SUM_SHFL=1 keeps __shfl_xor.
#ifndef GG_WAVE_SUM_SHFL
#define GG_WAVE_SUM_SHFL 0
#endif
__device__ __forceinline__ unsigned perm32_self(unsigned v)
{
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %0" : "+v"(v));
    return v;
}
__device__ __forceinline__ unsigned perm16_self(unsigned v)
{
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %0" : "+v"(v));
    return v;
}
template <int CTRL>
__device__ __forceinline__ double dpp64(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v)
{
    if constexpr (GG_WAVE_SUM_SHFL) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    } else {
        v += __hiloint2double((int)perm32_self((unsigned)__double2hiint(v)),
                              (int)perm32_self((unsigned)__double2loint(v)));
        v += __hiloint2double((int)perm16_self((unsigned)__double2hiint(v)),
                              (int)perm16_self((unsigned)__double2loint(v)));
        v += dpp64<0x128>(v);       // row_ror:8
        v += dpp64<0x124>(v);       // row_ror:4
        v += dpp64<0x122>(v);       // row_ror:2
        v += dpp64<0x121>(v);       // row_ror:1
        return v;
    }
}

// 256-thread block sum, result broadcast to every thread.
__device__ __forceinline__ double block_sum(double v)
{
    __shared__ double sh[kBlock / 64];
    __shared__ double res;
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) res = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    double r = res;
    __syncthreads();
    return r;
}

// block_sum with one barrier instead of three, the same bits (the same
// wave_sum per wave and (0 + 1) + (2 + 3)), every thread forming the sum from
// the four wave sums itself: the wave sums alternate between two LDS rows
// (`par`, uniform, flipped per call), so a call's writes never meet the
// previous call's reads -- between a call and the one after next there is
// always the barrier of the call in between.
__device__ __forceinline__ double block_sum_pp(double v, int &par)
{
    __shared__ double sh[2][kBlock / 64];
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[par][w] = v;
    __syncthreads();
    const double r = (sh[par][0] + sh[par][1]) + (sh[par][2] + sh[par][3]);
    par ^= 1;
    return r;
}

// block_sum of acc[k] for every k < nk at once, stored by thread k at
// part[k * kstride]: the same wave_sum per wave and (0 + 1) + (2 + 3) as
// block_sum, so the same bits, with one barrier instead of three per value.
// Once per kernel (its LDS is not re-armed).
template <int NK>
__device__ __forceinline__ void block_sum_store(const double (&acc)[NK], int nk, double *part, long long kstride)
{
    __shared__ double sh[kBlock / 64][NK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NK; k++) {
        if (k < nk) {
            const double v = wave_sum(acc[k]);
            if (lane == 0) sh[w][k] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < nk) {
        const int k = threadIdx.x;
        part[k * kstride] = (sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k]);
    }
}

// Sum of G per-block partials, identical (bit-for-bit) in every block.
__device__ __forceinline__ double sum_partials(const double *part, int G)
{
    double v = 0.0;
    for (int k = threadIdx.x; k < G; k += kBlock) v += part[k];
    return block_sum(v);
}

// UnitMap (kernels.h): does unit u (slots 2u, 2u+1) hold a real row?
__device__ __forceinline__ bool unit_real(const UnitMap &m, long long u)
{
    if (m.kind < 0) return true;
    if (m.kind == 0) return 2 * u < m.n;
    if (m.tbase) {
        if (u < m.tbase) return 2 * u < m.tn;
        u -= m.tbase;
    }
    const int lane = (int)(u & 63);
    const long long q = u >> 6;
    const int th = m.T >> 1;
    int j, k, lo;
    long long tp;
    if (m.kind == 1) {
        // 2D band layout (gg_internal.h Wave2D::slot): q = plane*nbands*T/2 + band*T/2 + t/2
        const long long per_plane = (long long)m.nbands * th;
        const long long kpl = q / per_plane;
        const long long r = q - kpl * per_plane;
        const int band = (int)(r / th);
        tp = r - (long long)band * th;
        j = band * 64 + lane;
        k = (int)kpl;
        lo = m.skew * lane + (m.skew - 1);              // the line's first real step
    } else {
        // 3D tiles: lane a + 8 g(c), t = i + a + c, band = K*NJ + J
        const long long band = q / th;
        tp = q - band * th;
        const int J = (int)(band % m.NJ), K = (int)(band / m.NJ);
        const int a = lane & 7, g = lane >> 3, c = g ^ (g >> 1) ^ (g >> 2);
        j = 8 * J + a;
        k = 8 * K + c;
        lo = a + c;
    }
    if (j >= m.ny || k >= m.nz) return false;
    const long long t0 = 2 * tp;
    return t0 + 1 >= lo && t0 < lo + m.nx;
}

// 16-B units a thread of the streaming kernels (per-step GMRES, CG, BiCGStab)
// loads per stream before it uses any
constexpr int kUnroll = 4;

__device__ __forceinline__ double2 ld2(const double *p, long long u)
{
    return reinterpret_cast<const double2 *>(p)[u];
}
// streamed once: non-temporal (does not displace re-used data from the caches)
typedef double dbl2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 ld2_nt(const double *p, long long u)
{
    const dbl2v v = __builtin_nontemporal_load(reinterpret_cast<const dbl2v *>(p) + u);
    return make_double2(v.x, v.y);
}
__device__ __forceinline__ void st2(double *p, long long u, double2 v)
{
    reinterpret_cast<double2 *>(p)[u] = v;
}

// ---- relaxed agent-scope loads/stores for the band hand-off --------------------
constexpr int kSpinLimit = 1 << 20;
// a wait this long (~10 ms of polls) only happens when a workgroup it waits on
// was never dispatched: persistent grids that were sized to be co-resident
// treat it as "not resident" and fall back (gather_first, k_trsv_tile3d)
constexpr int kResidSpin = 1 << 13;
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned long long *p, unsigned long long v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_agent_i(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent_i(int *p, int v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_agent_d(const double *p)
{
    return __longlong_as_double((long long)ld_agent(reinterpret_cast<const unsigned long long *>(p)));
}
__device__ __forceinline__ void st_agent_d(double *p, double v)
{
    st_agent(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v));
}

// ---- hand-offs inside one XCD ---------------------------------------------------
// A plain store (no sc bits) stops in the L2 of the XCD that issued it, where an
// agent-scope (sc1) poll from the same XCD finds it: 234 ns one way against 470
// for an sc1 store (profiles/r04/r04_xcd_handoff.txt).  Only for a reader known
// to run on the writer's XCD (HW_REG_XCC_ID of both): another XCD sees the
// value only once the line is written back.
constexpr int kXcds = 8;
__device__ __forceinline__ unsigned xcc_id()
{
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return v & (kXcds - 1);
}
__device__ __forceinline__ void st_plain(unsigned long long *p, unsigned long long v)
{
    asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(p), "v"(v) : "memory");
}

// 16 bytes stored write-through (two agent-scope 8-byte stores, sc1): visible
// to other XCDs once drained.  (Not inline asm: the compiler does not guard an
// asm store's data registers against the VALU write hazard that follows it.)
__device__ __forceinline__ void st_sc1_16(double2 *p, double2 v)
{
    unsigned long long *q = reinterpret_cast<unsigned long long *>(p);
    __hip_atomic_store(q, (unsigned long long)__double_as_longlong(v.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q + 1, (unsigned long long)__double_as_longlong(v.y), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

}  // namespace gg
