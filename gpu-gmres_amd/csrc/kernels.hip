// kernels.hip -- hand-written gfx950 (CDNA4) kernels for the GMRES hot path: the families that do not have
// a file of their own under kernels/ yet.
//
// Arithmetic order: every kernel that has a serial counterpart in the
// reference (SpMV row sums, triangular-solve rows, AXPY, Update) evaluates
// the same expression in the same order with contraction disabled
// (-ffp-contract=off), so it is bit-identical to the fp64 restatement.  Only
// the dot products / norms (wave-shuffle trees) round differently.
//
// Wave = 64 lanes; vector kernels use 256-thread blocks and 16-B (double2)
// loads; every reduction is a fixed tree (deterministic, no atomics).
#include "kernels/arnoldi.h"
#include "kernels/host.h"

namespace gg {

namespace {

// ============================================================== vector ops
__global__ void k_fill_u64(unsigned long long *p, long long n, unsigned long long v, long long zs = 0)
{
    p = zp(p, zs, blockIdx.y);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x)
        p[i] = v;
}

__global__ void k_gather(const double *in, const long long *idx, double *out, long long n,
                         unsigned long long *f0, unsigned long long *f1, long long nf)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        long long s = idx[i];
        out[i] = s < 0 ? 0.0 : in[s];
    }
    // (sentinel fills riding on the launch: the x arrays of a flow solve that follows)
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nf;
         i += (long long)gridDim.x * blockDim.x) {
        f0[i] = kSentinel;
        f1[i] = kSentinel;
    }
}

__global__ void k_copy(const double *in, double *out, long long units)
{
    for (long long u = blockIdx.x * (long long)blockDim.x + threadIdx.x; u < units;
         u += (long long)gridDim.x * blockDim.x)
        st2(out, u, ld2(in, u));
}

__global__ __launch_bounds__(kBlock) void k_dot(Gate g, const double *a, const double *b,
                                                double *part, long long units, long long zs = 0)
{
    // units: the dot range (a prefix of the vector space; the sharded solve
    // counts its separator replica on one shard only); zs: batched (blockIdx.y
    // = scenario, every operand per scenario)
    if (gated_z(g, zs, blockIdx.y)) return;
    a = zp(a, zs, blockIdx.y);
    b = zp(b, zs, blockIdx.y);
    part = zp(part, zs, blockIdx.y);
    double acc = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x; u0 < units; u0 += 4 * stride) {
        double2 x[4], y[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const long long u = u0 + j * stride;
            if (u < units) { x[j] = ld2(a, u); y[j] = ld2(b, u); }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (u0 + j * stride < units) {
                acc += x[j].x * y[j].x;
                acc += x[j].y * y[j].y;
            }
        }
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// ---- sharded solve (dd.hip) helpers ---------------------------------------------
// out[r] = in[r] - v_0 x[c_0] - v_1 x[c_1] - ...  in the listed (reference) order:
// the coupling terms a triangular row subtracts before its own triangle's terms
// (separator rows' interior terms, interior rows' separator terms)
// (f0, f1: nf words each set to the sentinel -- the x arrays of the two flow
// solves that follow, whose own fill launches this saves)
__global__ void k_sub_seq(Gate g, int n, const int *rp, const int *ci, const double *v,
                          const double *x, const double *in, double *out, unsigned long long *f0,
                          unsigned long long *f1, int nf)
{
    if (gated(g)) return;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        double acc = in[r];
        for (int k = rp[r]; k < rp[r + 1]; k++) acc -= v[k] * x[ci[k]];
        out[r] = acc;
    }
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nf; r += gridDim.x * blockDim.x) {
        if (f0) f0[r] = kSentinel;
        if (f1) f1[r] = kSentinel;
    }
}
// all shards of one process: slot s of shard s' buffer (at off + s*cnt) -> every other shard
__global__ void k_allgather_local(ShardPtrs b, int P, long long off, long long cnt)
{
    const long long tot = P * cnt;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < tot;
         e += (long long)gridDim.x * blockDim.x) {
        const int src = (int)(e / cnt);
        const double v = b.p[src][off + e];
        for (int q = 0; q < P; q++)
            if (q != src) b.p[q][off + e] = v;
    }
}
// k_allgather_local with each shard's slot gathered from its own vector in the
// same launch (kernels.h launch_gather_allgather_local)
__global__ void k_gather_allgather_local(ShardPtrs b, IdxPtrs gi, int P, long long off, long long cnt, FillPtrs fl,
                                         long long nf)
{
    const long long tot = P * cnt;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < tot;
         e += (long long)gridDim.x * blockDim.x) {
        const int src = (int)(e / cnt);
        const long long s = gi.p[src][e - src * cnt];
        const double v = s < 0 ? 0.0 : b.p[src][s];
        for (int q = 0; q < P; q++) b.p[q][off + e] = v;
    }
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nf;
         i += (long long)gridDim.x * blockDim.x) {
        for (int q = 0; q < P; q++) {
            if (fl.f0[q]) reinterpret_cast<unsigned long long *>(fl.f0[q])[i] = kSentinel;
            if (fl.f1[q]) reinterpret_cast<unsigned long long *>(fl.f1[q])[i] = kSentinel;
        }
    }
}
// GG_DD_IPC all-gather: one process per shard, every shard's exchange area
// mapped into every process (hipIpc; xGMI between GPUs).  Area of rank q:
// [flags: kMaxShards x kIpcXB u64][data: 2 parities x P slots x capd doubles].
// Block b owns chunk b of the cnt exchanged doubles: it stores the chunk of
// this rank's slot (buf + me*cnt) into every peer's data[seq & 1][me], releases
// flag[me][b] = seq at system scope in every peer's area, then waits (acquire,
// time-bounded) until every peer's flag[q][b] in this rank's area reached seq
// and copies those chunks to buf + q*cnt.  Sequence numbers only grow, so the
// flags are never re-armed; two parities suffice because a rank enters
// exchange k+1 only after every peer has entered exchange k, i.e. after it has
// finished copying out exchange k-1.  The area is uncached device memory
// (hipDeviceMallocUncached): remote stores and local polls need no cache
// maintenance beyond the system-scope release / acquire.
// gidx (k_ipc_gather_allgather's form): this rank's slot is gathered first,
// buf[me*cnt + e] = x[gidx[e]] (-1: 0), by the block that sends it
__global__ __launch_bounds__(kBlock) void k_ipc_allgather(IpcPeers pp, int me, int P, double *buf,
                                                          long long cnt, unsigned long long seq,
                                                          long long capd, int *err, const double *x,
                                                          const long long *gidx, unsigned long long *f0,
                                                          unsigned long long *f1, long long nf)
{
    const int nb = gridDim.x, b = blockIdx.x, t = threadIdx.x;
    const long long chunk = (cnt + nb - 1) / nb;
    const long long lo = (long long)b * chunk, hi = lo + chunk < cnt ? lo + chunk : cnt;
    const int par = (int)(seq & 1);
    constexpr long long kFlagWords = (long long)kMaxShards * kIpcXB;
    double *src = buf + (long long)me * cnt;
    if (gidx) {
        for (long long e = lo + t; e < hi; e += kBlock) {
            const long long s = gidx[e];
            src[e] = s < 0 ? 0.0 : x[s];
        }
    }
    for (long long i = b * (long long)kBlock + t; i < nf; i += (long long)nb * kBlock) {
        f0[i] = kSentinel;
        f1[i] = kSentinel;
    }
    for (int q = 0; q < P; q++) {
        if (q == me) continue;
        double *dst = reinterpret_cast<double *>(pp.base[q]) + kFlagWords + ((long long)par * P + me) * capd;
        for (long long e = lo + t; e < hi; e += kBlock) dst[e] = src[e];
    }
    __threadfence_system();
    __syncthreads();
    if (t < P && t != me) {
        unsigned long long *f = reinterpret_cast<unsigned long long *>(pp.base[t]) + (long long)me * kIpcXB + b;
        __hip_atomic_store(f, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        // wait for peer t's chunk b in this rank's area (bounded: ~30 s of the 100 MHz clock)
        const unsigned long long *w = reinterpret_cast<const unsigned long long *>(pp.base[me]) +
                                      (long long)t * kIpcXB + b;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(w, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < seq) {
            __builtin_amdgcn_s_sleep(2);
            if (__builtin_amdgcn_s_memrealtime() - t0 > 3000000000ull) {
                atomicOr(err, 4);
                break;
            }
        }
    }
    __syncthreads();
    for (int q = 0; q < P; q++) {
        if (q == me) continue;
        const double *rcv = reinterpret_cast<const double *>(pp.base[me]) + kFlagWords + ((long long)par * P + q) * capd;
        double *dst = buf + (long long)q * cnt;
        for (long long e = lo + t; e < hi; e += kBlock) dst[e] = rcv[e];
    }
}

// out[dst[i]] = in[src[i]]
__global__ void k_scatter_idx(const double *in, const long long *src, const long long *dst,
                              double *out, long long n)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x)
        out[dst[i]] = in[src[i]];
}

// ------------------------------------------------------- split (PG) maps
// MyILUPPfloat::DevPrecond_* elementwise steps (src/preconditioner.cu:1424-1558)
__global__ void k_mul(Gate g, const double *in, const double *s, double *out, int n)
{
    if (gated(g)) return;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] * s[i];
}
// the user-preconditioner boundary (fp32 arrays, src/preconditioner.h:34-84)
// order-independent fingerprint: sum of w_k * (2k + 1) over 32-bit words, mod 2^64
__global__ __launch_bounds__(kBlock) void k_fingerprint(const unsigned *p, long long nw, unsigned long long *out)
{
    unsigned long long acc = 0;
    for (long long k = blockIdx.x * (long long)kBlock + threadIdx.x; k < nw; k += (long long)gridDim.x * kBlock)
        acc += (unsigned long long)p[k] * (unsigned long long)(2 * k + 1);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);      // integer adds: any order, same sum
}

__global__ void k_f64_to_f32(Gate g, const double *in, float *out, int n)
{
    if (gated(g)) return;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}
__global__ void k_f32_to_f64(Gate g, const float *in, double *out, int n)
{
    if (gated(g)) return;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}
__global__ void k_div(Gate g, const double *in, const double *s, double *out, int n)
{
    if (gated(g)) return;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] / s[i];
}

// ================================================================= SpMV
// CSR-stream: a block owns <=256 consecutive rows holding <=kSpmvCap nnz.
// Products v*x[col] are formed with coalesced loads into LDS, then each row is
// summed serially in CSR order (computeSpMV order, src/SpMV_compute.cpp:19-36).
// YDIV: y[r] = (the row's result) / ydiv[r] -- the split engine's row gather
// and D_l scaling (gather_divsrc, src/preconditioner.cu:1592-1626) folded into
// the SpMV of the row-permuted matrix: the same division of the same value.
// XA: x read with agent-scope (sc1) loads -- values handed over inside the
// launch (k_dd_spmv_x's separator rows)
template <bool XA>
__device__ __forceinline__ double ld_x(const double *p)
{
    if constexpr (XA) return __longlong_as_double((long long)ld_agent(reinterpret_cast<const unsigned long long *>(p)));
    else return *p;
}
// YMUL: y[r] = (the row's result) * ymul[r] -- AINV's diagonal folded into its
// first product (MyAINV::HostPrecond's temp[i] = o_data[i] * diag_val[i])
template <bool RESID, bool YDIV, bool XA = false, bool YMUL = false>
__device__ __forceinline__ void spmv_stream_block(int bid, const int *blk, const int *rp, const int *ci,
                                                  const double *v, const double *x, const double *b, double *y,
                                                  const double *ydiv, const double *ymul = nullptr)
{
    constexpr int U = kSpmvCap / kBlock;        // products per thread
    __shared__ double prod[kSpmvCap];
    __shared__ int srp[kBlock + 1];
    const int tid = threadIdx.x;
    const int r0 = blk[bid], r1 = blk[bid + 1];
    const int nr = r1 - r0;                     // <= kBlock rows
    // the block's nr + 1 row pointers (nr <= kBlock: the last one by thread 0)
    if (tid < nr) srp[tid] = rp[r0 + tid];
    if (tid == 0) srp[nr] = rp[r1];
    __syncthreads();
    const int e0 = srp[0], e1 = srp[nr];
    const int cnt = e1 - e0;
    if (cnt > kSpmvCap) {   // one long row: strided partial sums + tree
        double acc = 0.0;
        for (int e = e0 + tid; e < e1; e += kBlock) acc += v[e] * ld_x<XA>(x + ci[e]);
        acc = block_sum(acc);
        if (tid == 0) {
            const double o = RESID ? (-1.0 * acc + 1.0 * b[r0]) : acc;
            y[r0] = YDIV ? o / ydiv[r0] : YMUL ? o * ymul[r0] : o;
        }
        return;
    }
    // entries in aligned pairs (8-B index and 16-B value loads) from the even
    // entry at or below e0; all index/value loads first, then all gathers
    constexpr int U2 = U / 2 + 1;               // pairs per thread (the alignment adds one)
    const int ea = e0 & ~1;
    const int npair = (e1 - ea + 1) >> 1;
    int2 c[U2];
    double2 vv[U2], xv[U2];
#pragma unroll
    for (int u = 0; u < U2; u++) {
        const int p = tid + u * kBlock;
        if (p < npair) {
            c[u] = reinterpret_cast<const int2 *>(ci + ea)[p];
            vv[u] = reinterpret_cast<const double2 *>(v + ea)[p];
        }
    }
#pragma unroll
    for (int u = 0; u < U2; u++) {
        const int p = tid + u * kBlock;
        const int e = ea + 2 * p;
        if (p < npair) {
            if (e >= e0) xv[u].x = ld_x<XA>(x + c[u].x);
            if (e + 1 < e1) xv[u].y = ld_x<XA>(x + c[u].y);
        }
    }
#pragma unroll
    for (int u = 0; u < U2; u++) {
        const int p = tid + u * kBlock;
        const int e = ea + 2 * p;
        if (p < npair) {
            if (e >= e0) prod[e - e0] = vv[u].x * xv[u].x;
            if (e + 1 < e1) prod[e + 1 - e0] = vv[u].y * xv[u].y;
        }
    }
    __syncthreads();
    if (tid < nr) {
        // the row's products in CSR order; eight LDS reads in flight per
        // group (a read-then-add loop waits an LDS round trip per term)
        double acc = 0.0;
        const int a = srp[tid] - e0, z = srp[tid + 1] - e0;
        int e = a;
        for (; e + 8 <= z; e += 8) {
            double t[8];
#pragma unroll
            for (int q = 0; q < 8; q++) t[q] = prod[e + q];
#pragma unroll
            for (int q = 0; q < 8; q++) acc += t[q];
        }
        for (; e < z; e++) acc += prod[e];
        const int r = r0 + tid;
        const double o = RESID ? (-1.0 * acc + 1.0 * b[r]) : acc;
        y[r] = YDIV ? o / ydiv[r] : YMUL ? o * ymul[r] : o;
    }
}
template <bool RESID, bool YDIV = false>
__global__ __launch_bounds__(kBlock) void k_spmv_stream(Gate g, const int *blk, const int *rp,
                                                        const int *ci, const double *v,
                                                        const double *x, const double *b,
                                                        double *y, const double *ydiv)
{
    if (gated(g)) return;
    spmv_stream_block<RESID, YDIV>(blockIdx.x, blk, rp, ci, v, x, b, y, ydiv);
}
// y = (A x) o ymul
__global__ __launch_bounds__(kBlock) void k_spmv_stream_mul(Gate g, const int *blk, const int *rp, const int *ci,
                                                            const double *v, const double *x, double *y,
                                                            const double *ymul)
{
    if (gated(g)) return;
    spmv_stream_block<false, false, false, true>(blockIdx.x, blk, rp, ci, v, x, nullptr, y, nullptr, ymul);
}

// Sliced ELL: one wave per 64-row slice, lane = row; the slice's entries are
// read k-major (each load instruction is one coalesced 256-B / 512-B line per
// wave), up to 8 index/value pairs in flight before their gathers; each row is
// summed serially in CSR order from 0.0, skipping the padding (col -1): the
// same operations as k_spmv_stream (computeSpMV order).
// GG_SPMV_XCD: blocks b, b+8, ... (one XCD under round-robin dispatch, for
// speed only) take consecutive slices, so the x lines that neighbouring slices
// share are fetched into one L2 (the 3D tile layout's line and plane
// neighbours are 64 and 13,824 rows away)
#ifndef GG_SPMV_XCD
#define GG_SPMV_XCD 1
#endif
__device__ __forceinline__ int xcd_block()
{
    if (!GG_SPMV_XCD) return blockIdx.x;
    const int nb = gridDim.x, q = nb >> 3, rem = nb & 7, x = blockIdx.x & 7;
    return x * q + (x < rem ? x : rem) + (blockIdx.x >> 3);
}

// XDIV: x[c] = RN(x[c] / xdiv[c]) formed per gathered term -- the split
// engine's D_r^-1 pass (k_div) folded into the gathers, the same division
// YMUL: y[r] = (the row's result) * ymul[r] (AINV's diagonal)
template <bool RESID, bool YDIV, bool XDIV, bool XA = false, bool YMUL = false>
__device__ __forceinline__ void spmv_sell_slice(int s, int n, const int *sptr, const int *__restrict__ ci,
                                                const double *__restrict__ v, const double *x,
                                                const double *__restrict__ b, double *__restrict__ y,
                                                const double *__restrict__ ydiv, const double *__restrict__ xdiv,
                                                const double *__restrict__ ymul = nullptr)
{
    const int lane = threadIdx.x & 63;
    const int off = sptr[s], w = (sptr[s + 1] - off) >> 6;
    const int *cp = ci + off + lane;
    const double *vp = v + off + lane;
    double acc = 0.0;
    for (int k0 = 0; k0 < w; k0 += 8) {
        int c[8];
        double a[8], xv[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k0 + k < w) {
                c[k] = __builtin_nontemporal_load(cp + (k0 + k) * 64);
                a[k] = __builtin_nontemporal_load(vp + (k0 + k) * 64);
            }
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k0 + k < w && c[k] >= 0) xv[k] = ld_x<XA>(x + c[k]);
        if constexpr (XDIV) {
            double dv[8];
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (k0 + k < w && c[k] >= 0) dv[k] = xdiv[c[k]];
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (k0 + k < w && c[k] >= 0) xv[k] = xv[k] / dv[k];
        }
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k0 + k < w && c[k] >= 0) acc += a[k] * xv[k];
    }
    const int r = s * 64 + lane;
    if (r < n) {
        const double o = RESID ? (-1.0 * acc + 1.0 * b[r]) : acc;
        y[r] = YDIV ? o / ydiv[r] : YMUL ? o * ymul[r] : o;
    }
}
template <bool RESID, bool YDIV = false, bool XDIV = false>
__global__ __launch_bounds__(kBlock) void k_spmv_sell(Gate g, int n, int nslice, const int *sptr,
                                                      const int *__restrict__ ci,
                                                      const double *__restrict__ v,
                                                      const double *__restrict__ x,
                                                      const double *__restrict__ b,
                                                      double *__restrict__ y,
                                                      const double *__restrict__ ydiv,
                                                      const double *__restrict__ xdiv,
                                                      unsigned long long *fill = nullptr, int nfill = 0)
{
    // (XDIV, fill: the next flow solve's x set to the sentinel, rows < nfill --
    // the k_fill_gated launch that solve would make)
    if (gated(g)) return;
    const int s = xcd_block() * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= nslice) return;
    if constexpr (XDIV) {
        const int r = s * 64 + (int)(threadIdx.x & 63);
        if (fill && r < nfill) fill[r] = kSentinel;
    }
    spmv_sell_slice<RESID, YDIV, XDIV>(s, n, sptr, ci, v, x, b, y, ydiv, xdiv);
}
// y = (A x) o ymul
__global__ __launch_bounds__(kBlock) void k_spmv_sell_mul(Gate g, int n, int nslice, const int *sptr,
                                                          const int *__restrict__ ci, const double *__restrict__ v,
                                                          const double *__restrict__ x, double *__restrict__ y,
                                                          const double *__restrict__ ymul)
{
    if (gated(g)) return;
    const int s = xcd_block() * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= nslice) return;
    spmv_sell_slice<false, false, false, false, true>(s, n, sptr, ci, v, x, nullptr, y, nullptr, nullptr, ymul);
}

// Column-panel SpMV, one launch per panel p (DevCsr::panel): a block owns a
// run of <= 256 of the panel's row segments (a row's terms whose columns fall
// in the panel, in CSR order) holding <= kSpmvCap entries (pblk, host-made),
// and works like k_spmv_stream on it -- entries loaded coalesced, x gathered
// (from the panel's slice, which the XCD's L2 keeps), products into LDS, then
// each segment's products summed by its thread in order, continuing the row's
// running sum kept in y (0.0 at the row's first segment, seg_row = ~row).
// Every row is thus summed exactly as computeSpMV sums it.  Empty rows get 0
// in pass 0.  GG_PANEL_NT=1: the panel's entries and segment tables streamed
// non-temporally, so that they do not push the x slice out of the L2.
// (C3 stand-in, one box, profiles/r06/c3_panel_ab.txt: 648 -> 640 us at 4 MiB
// panels, 651 -> 626 us at 6 MiB)
#ifndef GG_PANEL_NT
#define GG_PANEL_NT 1
#endif
template <class T>
__device__ __forceinline__ T pan_ld(const T *p)
{
    if constexpr (GG_PANEL_NT) return __builtin_nontemporal_load(p);
    else return *p;
}
// one sub-block (<= 256 segments, <= kSpmvCap entries) of the panel layout;
// YA: the running sums read with agent-scope loads (k_spmv_rtile: the row's
// previous segment was stored by this block, by another of its threads)
template <bool YA>
__device__ __forceinline__ void panel_subblock(int sb, const int *__restrict__ pblk, const int *__restrict__ seg_row,
                                               const int *__restrict__ seg_ptr, const int *__restrict__ pci,
                                               const double *__restrict__ pv, const double *__restrict__ x, double *y)
{
    constexpr int U = kSpmvCap / kBlock;        // entries per thread
    __shared__ double prod[kSpmvCap];
    __shared__ int sp[kBlock + 1];
    const int tid = threadIdx.x;
    const int s0 = pblk[sb], s1 = pblk[sb + 1];
    const int ns = s1 - s0;                     // <= kBlock segments
    if (tid < ns) sp[tid] = pan_ld(seg_ptr + s0 + tid);
    if (tid == 0) sp[ns] = pan_ld(seg_ptr + s1);
    int rr = 0;
    double acc = 0.0;
    if (tid < ns) {
        rr = pan_ld(seg_row + s0 + tid);
        if (rr >= 0) acc = ld_x<YA>(y + rr);    // the row's running sum so far
    }
    __syncthreads();
    const int e0 = sp[0], cnt = sp[ns] - e0;
    int c[U];
    double a[U], xv[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int q = tid + u * kBlock;
        if (q < cnt) {
            c[u] = pan_ld(pci + e0 + q);
            a[u] = pan_ld(pv + e0 + q);
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++)
        if (tid + u * kBlock < cnt) xv[u] = x[c[u]];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int q = tid + u * kBlock;
        if (q < cnt) prod[q] = a[u] * xv[u];
    }
    __syncthreads();
    if (tid < ns) {
        const int lo = sp[tid] - e0, hi = sp[tid + 1] - e0;
        int e = lo;
        for (; e + 8 <= hi; e += 8) {
            double t[8];
#pragma unroll
            for (int q = 0; q < 8; q++) t[q] = prod[e + q];
#pragma unroll
            for (int q = 0; q < 8; q++) acc += t[q];
        }
        for (; e < hi; e++) acc += prod[e];
        y[rr < 0 ? ~rr : rr] = acc;
    }
}
__global__ __launch_bounds__(kBlock) void k_spmv_panel(Gate g, const int *__restrict__ pblk,
                                                       const int *__restrict__ seg_row,
                                                       const int *__restrict__ seg_ptr,
                                                       const int *__restrict__ pci, const double *__restrict__ pv,
                                                       const double *__restrict__ x, double *__restrict__ y,
                                                       const int *__restrict__ zero_rows, int nzero)
{
    if (gated(g)) return;
    if (nzero)
        for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < nzero; i += (long long)gridDim.x * kBlock)
            y[zero_rows[i]] = 0.0;
    panel_subblock<false>(blockIdx.x, pblk, seg_row, seg_ptr, pci, pv, x, y);
}
// Row tiles (DevCsr::rtile): ONE launch, block b walking its sub-blocks
// rt_sub[b] .. rt_sub[b+1]-1 in order -- its rows' segments panel by panel, so
// a row's terms are added in column order (the CSR order: the same bits), its
// running sum in y only ever touched by this block.  Between sub-blocks the
// y stores are drained and the block synchronises; the next sub-block reads y
// with agent-scope loads (past this CU's L1).
__global__ __launch_bounds__(kBlock) void k_spmv_rtile(Gate g, const int *__restrict__ rt_sub,
                                                       const int *__restrict__ pblk,
                                                       const int *__restrict__ seg_row,
                                                       const int *__restrict__ seg_ptr,
                                                       const int *__restrict__ pci, const double *__restrict__ pv,
                                                       const double *__restrict__ x, double *y,
                                                       const int *__restrict__ zero_rows, int nzero)
{
    if (gated(g)) return;
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < nzero; i += (long long)gridDim.x * kBlock)
        y[zero_rows[i]] = 0.0;
    const int b0 = rt_sub[blockIdx.x], b1 = rt_sub[blockIdx.x + 1];
    for (int sb = b0; sb < b1; sb++) {
        panel_subblock<true>(sb, pblk, seg_row, seg_ptr, pci, pv, x, y);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this sub-block's y stores done
        __syncthreads();
    }
}

// The sharded SpMV with its interface exchange in ONE launch (dd.hip
// spmv_rows; GG_DD_IPC / GG_DD_LOOPBACK, one shard per process): north_star's
// overlap of the halo exchange with the interior rows, without a second
// stream and its cross-stream event pair.
//   blocks [0, nbx): the exchange -- k_ipc_allgather's protocol with this
//     rank's slot gathered in the launch (IPC), or the loopback all-gather over
//     this shard's own buffer (LOOPBACK, timing only: k_gather_allgather_local's
//     stores); every halo value is stored write-through (sc1), each storing wave
//     drains its stores, and after a barrier one lane adds 1 to *arrived
//   blocks [nbx, nbx + nbi): the interior rows (they read no halo value)
//   blocks after: the separator rows; one lane waits for *arrived >= target,
//     the block passes a barrier, then reads x with agent-scope loads only
//     (MI355X_MICROARCH.md's hand-off table, row 1)
// A block waits only on blocks of lower index (dispatched first).  Each row's
// operations are k_spmv_sell's / k_spmv_stream's: the same bits as the
// unfused launches.
template <bool RESID>
__global__ __launch_bounds__(kBlock) void k_dd_spmv_x(Gate g, DdSpmvX a)
{
    const int bid = blockIdx.x, t = threadIdx.x;
    if (bid < a.nbx) {
        const int nb = a.nbx;
        if (a.loop) {
            // loopback: slot q of the halo = this shard's own interface values
            const long long tot = (long long)a.P * a.cnt;
            for (long long e = bid * (long long)kBlock + t; e < tot; e += (long long)nb * kBlock) {
                const long long sq = a.gidx[e % a.cnt];
                const double v = sq < 0 ? 0.0 : a.x[sq];
                st_agent(reinterpret_cast<unsigned long long *>(a.halo + e), (unsigned long long)__double_as_longlong(v));
            }
        } else {
            const long long chunk = (a.cnt + nb - 1) / nb;
            const long long lo = (long long)bid * chunk, hi = lo + chunk < a.cnt ? lo + chunk : a.cnt;
            const int par = (int)(a.seq & 1);
            constexpr long long kFlagWords = (long long)kMaxShards * kIpcXB;
            double *src = a.halo + (long long)a.me * a.cnt;
            for (long long e = lo + t; e < hi; e += kBlock) {
                const long long sq = a.gidx[e];
                const double v = sq < 0 ? 0.0 : a.x[sq];
                st_agent(reinterpret_cast<unsigned long long *>(src + e), (unsigned long long)__double_as_longlong(v));
                for (int q = 0; q < a.P; q++) {
                    if (q == a.me) continue;
                    double *dst = reinterpret_cast<double *>(a.pp.base[q]) + kFlagWords + ((long long)par * a.P + a.me) * a.capd;
                    dst[e] = v;
                }
            }
            __threadfence_system();
            __syncthreads();
            if (t < a.P && t != a.me) {
                unsigned long long *f = reinterpret_cast<unsigned long long *>(a.pp.base[t]) + (long long)a.me * kIpcXB + bid;
                __hip_atomic_store(f, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                const unsigned long long *w = reinterpret_cast<const unsigned long long *>(a.pp.base[a.me]) +
                                              (long long)t * kIpcXB + bid;
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                while (__hip_atomic_load(w, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < a.seq) {
                    __builtin_amdgcn_s_sleep(2);
                    if (__builtin_amdgcn_s_memrealtime() - t0 > 3000000000ull) {
                        atomicOr(a.err, 4);
                        break;
                    }
                }
            }
            __syncthreads();
            for (int q = 0; q < a.P; q++) {
                if (q == a.me) continue;
                const double *rcv =
                    reinterpret_cast<const double *>(a.pp.base[a.me]) + kFlagWords + ((long long)par * a.P + q) * a.capd;
                double *dst = a.halo + (long long)q * a.cnt;
                for (long long e = lo + t; e < hi; e += kBlock)
                    st_agent(reinterpret_cast<unsigned long long *>(dst + e),
                             (unsigned long long)__double_as_longlong(rcv[e]));
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every wave's halo stores drained
        __syncthreads();
        if (t == 0) __hip_atomic_fetch_add(a.arrived, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (gated(g)) return;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    if (bid < a.nbx + a.nbi) {
        const int q = bid - a.nbx;
        if (a.i_sell) {
            const int sl = q * (kBlock / 64) + wv;
            if (sl < a.i_nb) spmv_sell_slice<RESID, false, false>(sl, a.i_n, a.i_ptr, a.i_ci, a.i_v, a.x, a.b, a.y,
                                                                  nullptr, nullptr);
        } else {
            spmv_stream_block<RESID, false>(q, a.i_ptr, a.i_rp, a.i_ci, a.i_v, a.x, a.b, a.y, nullptr);
        }
        return;
    }
    if (t == 0) {
        int spins = 0;
        while (ld_agent(a.arrived) < a.target) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > kSpinLimit * 16) {
                atomicOr(a.err, 4);
                break;
            }
        }
    }
    __syncthreads();
    const int q = bid - a.nbx - a.nbi;
    const double *bs = RESID ? a.b + a.S0 : nullptr;
    double *ys = a.y + a.S0;
    if (a.s_sell) {
        const int sl = q * (kBlock / 64) + wv;
        if (sl < a.s_nb) spmv_sell_slice<RESID, false, false, true>(sl, a.s_n, a.s_ptr, a.s_ci, a.s_v, a.x, bs, ys,
                                                                    nullptr, nullptr);
    } else {
        spmv_stream_block<RESID, false, true>(q, a.s_ptr, a.s_rp, a.s_ci, a.s_v, a.x, bs, ys, nullptr);
    }
}

// Batched SpMV (the many-RHS solve): y_sc = A x_sc (RESID: b_sc - A x_sc) for
// up to NS scenarios per launch (scenario sc's vectors sc * zs bytes after
// scenario 0's), A's sliced-ELL entries read ONCE per wave for all of them.
// Every row of every scenario is summed exactly as k_spmv_sell sums it (entry
// order from 0.0, no contraction): the same bits.  A scenario whose gate is
// closed (converged) is skipped.
template <bool RESID, int NS>
__global__ __launch_bounds__(kBlock) void k_spmv_sell_b(Gate g, long long zs, int nsc, int n, int nslice,
                                                        const int *sptr, const int *__restrict__ ci,
                                                        const double *__restrict__ v, const double *x,
                                                        const double *b, double *y)
{
    const int s = xcd_block() * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= nslice) return;
    bool act[NS];
    bool any = false;
#pragma unroll
    for (int q = 0; q < NS; q++) {
        act[q] = q < nsc && !gated_z(g, zs, q);
        any |= act[q];
    }
    if (!any) return;
    const int lane = threadIdx.x & 63;
    const int off = sptr[s], w = (sptr[s + 1] - off) >> 6;
    const int *cp = ci + off + lane;
    const double *vp = v + off + lane;
    double acc[NS];
#pragma unroll
    for (int q = 0; q < NS; q++) acc[q] = 0.0;
    for (int k0 = 0; k0 < w; k0 += 8) {
        int c[8];
        double a[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k0 + k < w) {
                c[k] = __builtin_nontemporal_load(cp + (k0 + k) * 64);
                a[k] = __builtin_nontemporal_load(vp + (k0 + k) * 64);
            }
#pragma unroll
        for (int q = 0; q < NS; q++) {
            if (!act[q]) continue;
            const double *xq = zp(x, zs, q);
            double xv[8];
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (k0 + k < w && c[k] >= 0) xv[k] = xq[c[k]];
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (k0 + k < w && c[k] >= 0) acc[q] += a[k] * xv[k];
        }
    }
    const int r = s * 64 + lane;
    if (r < n) {
#pragma unroll
        for (int q = 0; q < NS; q++) {
            if (!act[q]) continue;
            zp(y, zs, q)[r] = RESID ? (-1.0 * acc[q] + 1.0 * zp(b, zs, q)[r]) : acc[q];
        }
    }
}

// ======================================================= triangular solves
// Level-scheduled row solve (one launch per dependency level):
//   x[r] = (b[r] - sum_k off[k] * x[col[k]]) / d[r]   in canonical order
// y (optional): RN(1/d) -- x = RN(acc * y), WD_MUL's row (a bordered grid's
// tail under gg_set_division(GG_DIV_RCP), DevTri::tail).  fm: GG_DIV_FMA's row
// (a bordered grid's tail, DevTri::tail_fma): acc = RN(b * y) (b when y is null),
// then acc = fma(-v, x, acc) over the terms as stored -- pre-scaled by y and in
// the fused order (nearest first) -- and no division
__global__ __launch_bounds__(kBlock) void k_trsv_level(Gate g, int cnt, const int *rows,
                                                       const int *rp, const int *ci,
                                                       const double *v, const double *d,
                                                       const double *b, double *x, const double *y, int fm)
{
    if (gated(g)) return;
    int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= cnt) return;
    int r = rows[t];
    if (fm) {                       // GG_DIV_FMA's rows (the terms pre-scaled and in fused order)
        double acc = y ? b[r] * y[r] : b[r];
        for (int k = rp[r]; k < rp[r + 1]; k++) acc = __builtin_fma(-v[k], x[ci[k]], acc);
        x[r] = acc;
        return;
    }
    double acc = b[r];
    for (int k = rp[r]; k < rp[r + 1]; k++) acc = acc - v[k] * x[ci[k]];
    x[r] = y ? acc * y[r] : acc / d[r];
}

// Sync-free (dataflow) form of the same solve, one launch per triangle: x is
// pre-filled with the sentinel and a row's value is its own ready flag.  Rows
// are taken in level order (lev_rows), a wave 64 consecutive ones, the
// co-resident grid striding over the list; a lane loads all its sources with
// agent-scope loads, and if none is the sentinel finishes the row with the
// same operations as k_trsv_level (canonical order, then / d[r]) and stores it
// with an agent-scope store; otherwise it retries inside a wave-uniform loop
// (sources of one wave's rows may be other lanes of the wave).  The smallest
// unfinished row in level order always has its sources done, so the grid
// drains; spins are bounded (err bit 0).
__global__ void k_fill_gated(Gate g, unsigned long long *p, long long n, unsigned long long v)
{
    if (gated(g)) return;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        p[i] = v;
}

// long rows: issue the next round's loads before this round's serial sum (1;
// 92 VGPRs, 5 waves per SIMD) or after it (0; 62 VGPRs, 8 waves per SIMD)
#ifndef GG_FLOW_PREFETCH
#define GG_FLOW_PREFETCH 1
#endif
// one long row (more than kFlowLong terms), the whole wave: each round 256 of
// its terms (4 per lane) are loaded and polled together, their products v*x
// formed in parallel, then lane 0 subtracts them from acc one by one in
// canonical order -- the reference's serial arithmetic
__device__ __forceinline__ void flow_long_row(int r, const int *__restrict__ rp, const int *__restrict__ ci,
                                              const double *__restrict__ v, const double *__restrict__ d,
                                              const double *__restrict__ b, unsigned long long *xu, int *err,
                                              const double *__restrict__ y, double *wprod, int lane)
{
    const int k0 = rp[r], k1 = rp[r + 1];
    double acc = b[r];
    int spins = 0;
    // round kc's columns, coefficients and x polls; the next round's
    // are issued before this round's serial sum (their latency hidden)
    int c[4];
    double vv[4];
    unsigned long long u[4];
    auto fetch = [&](int kc, int *cc, double *vc, unsigned long long *uc) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = kc + q * 64 + lane;
            cc[q] = k < k1 ? ci[k] : -1;
            vc[q] = k < k1 ? v[k] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) uc[q] = cc[q] >= 0 ? ld_agent(xu + cc[q]) : 0ull;
    };
    fetch(k0, c, vv, u);
    for (int kc = k0; kc < k1; kc += 256) {
        if (!GG_FLOW_PREFETCH && kc > k0) fetch(kc, c, vv, u);
        while (true) {
            bool miss = false;
#pragma unroll
            for (int q = 0; q < 4; q++) miss |= c[q] >= 0 && u[q] == kSentinel;
            if (!__any(miss)) break;
            __builtin_amdgcn_s_sleep(2);
            if (++spins > kSpinLimit) {
                if (lane == 0) atomicOr(err, 1);
                break;
            }
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (c[q] >= 0 && u[q] == kSentinel) u[q] = ld_agent(xu + c[q]);
        }
        double pq[4];
#pragma unroll
        for (int q = 0; q < 4; q++) pq[q] = vv[q] * __longlong_as_double((long long)u[q]);
        if (GG_FLOW_PREFETCH && kc + 256 < k1) fetch(kc + 256, c, vv, u);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            wprod[lane] = pq[q];
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            const int cnt = k1 - (kc + q * 64);
            if (lane == 0) {
                // the 64 products in canonical order, read 8 at a time one
                // chunk ahead (a read-then-subtract loop waits an LDS round
                // trip per term)
                const double2 *wp2 = reinterpret_cast<const double2 *>(wprod);
                double2 cur[4], nxt[4];
#pragma unroll
                for (int e = 0; e < 4; e++) cur[e] = wp2[e];
#pragma unroll
                for (int c8 = 0; c8 < 8; c8++) {
                    if (c8 + 1 < 8) {
#pragma unroll
                        for (int e = 0; e < 4; e++) nxt[e] = wp2[(c8 + 1) * 4 + e];
                    }
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int j = c8 * 8 + 2 * e;
                        if (j < cnt) acc = acc - cur[e].x;
                        if (j + 1 < cnt) acc = acc - cur[e].y;
                    }
#pragma unroll
                    for (int e = 0; e < 4; e++) cur[e] = nxt[e];
                }
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }
    }
    if (lane == 0) st_agent(xu + r, (unsigned long long)__double_as_longlong(y ? acc * y[r] : acc / d[r]));
}

// ELL: short rows read their terms from the sliced copy (DevTri::eci / ev,
// task {.z, .w}) instead of rp / ci / v: no rp -> ci -> poll chain of dependent
// loads, one coalesced load per term index; the operations are the same (pgr:
// L 84.0 -> 62.8, U 103.0 -> 68.9 us, profiles/r04/r04y_pgr_e*.json; a software-
// pipelined task loop -- the next task's loads behind this one's polls --
// measured 67.1 / 73.1 us, r04z_pgr_e1.json, not kept).
// s_sleep between a wave's poll rounds while a lane waits on a source
#ifndef GG_FLOW_SLEEP
#define GG_FLOW_SLEEP 4
#endif
// how a short row's lane polls its sources (x pre-filled with the sentinel,
// each slot written once per launch: a value other than the sentinel is final)
//   0: every round re-loads the chunk's sources from the first unconsumed one
//   1: a source seen ready is kept in a register; only sentinel ones re-polled
//   2: as 1, and each source's first probe is a PLAIN load (L1/L2-served: a
//      stale copy can only show the sentinel, which falls back to the agent poll)
#ifndef GG_FLOW_POLL
#define GG_FLOW_POLL 1
#endif
__device__ __forceinline__ unsigned long long ld_flow_first(const unsigned long long *p)
{
    if constexpr (GG_FLOW_POLL == 2) return *reinterpret_cast<const volatile unsigned long long *>(p);
    else return ld_agent(p);
}
template <bool ELL>
__global__ __launch_bounds__(kBlock) void k_trsv_flow(Gate g, int ntask, const int4 *__restrict__ tasks,
                                                      const int *__restrict__ rows,
                                                      const int *__restrict__ rp, const int *__restrict__ ci,
                                                      const double *__restrict__ v,
                                                      const double *__restrict__ d,
                                                      const double *__restrict__ b, double *x, int *err,
                                                      const double *__restrict__ y, int fm,
                                                      const int *__restrict__ eci, const double *__restrict__ ev)
{
    if (gated(g)) return;
    __shared__ double prod[kBlock];            // a long row's products, one 64-slot area per wave
    const int lane = threadIdx.x & 63;
    double *wprod = prod + (threadIdx.x & ~63);
    const long long wid = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
    const long long nw = (gridDim.x * (long long)blockDim.x) >> 6;
    unsigned long long *xu = reinterpret_cast<unsigned long long *>(x);
    for (long long t = wid; t < ntask; t += nw) {
        const int4 tk = tasks[t];
        if (tk.y < 0) {
            // (fm triangles are built without long rows: build_tri_bordered)
            flow_long_row(rows[tk.x], rp, ci, v, d, b, xu, err, y, wprod, lane);
            continue;
        }
        if constexpr (ELL) {
            // up to 64 short rows, one per lane, terms from the sliced copy four
            // at a time (cc / vv: terms kb .. kb+3; column -1 past the row's end)
            const int r = lane < tk.y ? rows[tk.x + lane] : -1;
            const int w = tk.w;
            const long long eb = (long long)tk.z * 64 + lane;
            int cc[4];
            double vv[4];
            auto chunk = [&](int kb) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    cc[j] = kb + j < w ? eci[eb + (long long)(kb + j) * 64] : -1;
                    vv[j] = kb + j < w ? ev[eb + (long long)(kb + j) * 64] : 0.0;
                }
            };
            chunk(0);
            bool pending = r >= 0;
            // y: the reciprocal (WD_MUL's row; fm: b's pre-scale, GG_DIV_FMA's row)
            double acc = pending ? ((fm && y) ? b[r] * y[r] : b[r]) : 0.0;
            const double dr = pending ? (y ? y[r] : d[r]) : 1.0;
            int kb = 0, k = 0;                  // chunk base, terms consumed
            int spins = 0;
            unsigned long long u[4];            // GG_FLOW_POLL >= 1: the chunk's sources as last seen
            bool fresh = true;                  // the chunk not probed yet
            while (__any(pending)) {
                if (pending) {
                    // consume the sources in canonical order as far as they
                    // are ready (a source once seen stays final)
                    while (true) {
                        if constexpr (GG_FLOW_POLL == 0) {
#pragma unroll
                            for (int j = 0; j < 4; j++) u[j] = (kb + j >= k && cc[j] >= 0) ? ld_agent(xu + cc[j]) : 0ull;
                        } else if (fresh) {
#pragma unroll
                            for (int j = 0; j < 4; j++) u[j] = (kb + j >= k && cc[j] >= 0) ? ld_flow_first(xu + cc[j]) : 0ull;
                            fresh = false;
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; j++)
                                if (kb + j >= k && cc[j] >= 0 && u[j] == kSentinel) u[j] = ld_agent(xu + cc[j]);
                        }
                        bool stop = false;
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            if (!stop && kb + j >= k && cc[j] >= 0) {
                                if (u[j] == kSentinel) {
                                    stop = true;
                                } else {
                                    const double xj = __longlong_as_double((long long)u[j]);
                                    acc = fm ? __builtin_fma(-vv[j], xj, acc) : acc - vv[j] * xj;
                                    k++;
                                }
                            }
                        }
                        if (stop) break;
                        if (cc[3] < 0 || kb + 4 >= w) {
                            st_agent(xu + r, (unsigned long long)__double_as_longlong(fm ? acc : y ? acc * dr : acc / dr));
                            pending = false;
                            break;
                        }
                        kb += 4;
                        chunk(kb);
                        fresh = true;
                    }
                }
                if (__any(pending)) {
                    __builtin_amdgcn_s_sleep(GG_FLOW_SLEEP);
                    if (++spins > kSpinLimit) {
                        if (pending) atomicOr(err, 1);
                        pending = false;
                    }
                }
            }
            continue;
        }
        // up to 64 short rows, one per lane
        const int r = lane < tk.y ? rows[tk.x + lane] : -1;
        bool pending = r >= 0;
        int k = pending ? rp[r] : 0;
        const int k1 = pending ? rp[r + 1] : 0;
        // y: the reciprocal (WD_MUL's row; fm: b's pre-scale, GG_DIV_FMA's row)
        double acc = pending ? ((fm && y) ? b[r] * y[r] : b[r]) : 0.0;
        const double dr = pending ? (y ? y[r] : d[r]) : 1.0;
        int spins = 0;
        unsigned long long u[4];                // GG_FLOW_POLL >= 1: sources k .. k+3 as last seen
        int ub = -1;                            // the k they were loaded for (-1: none)
        while (__any(pending)) {
            if (pending) {
                // consume the sources in canonical order as far as they are
                // ready (one outstanding poll per waiting lane); a source
                // once seen stays final, so acc is built incrementally
                bool stop = false;
                while (!stop && k < k1) {
                    // up to 4 polls in flight
                    if (GG_FLOW_POLL == 0) {
#pragma unroll
                        for (int j = 0; j < 4; j++) u[j] = k + j < k1 ? ld_agent(xu + ci[k + j]) : 0ull;
                    } else if (ub != k) {
#pragma unroll
                        for (int j = 0; j < 4; j++) u[j] = k + j < k1 ? ld_flow_first(xu + ci[k + j]) : 0ull;
                        ub = k;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            if (k + j < k1 && u[j] == kSentinel) u[j] = ld_agent(xu + ci[k + j]);
                    }
                    const int k0 = k;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (stop || k >= k1) break;
                        if (u[j] == kSentinel) { stop = true; break; }
                        const double xj = __longlong_as_double((long long)u[j]);
                        acc = fm ? __builtin_fma(-v[k], xj, acc) : acc - v[k] * xj;
                        k++;
                    }
                    if (stop && k != k0) {
                        // sources k0 .. k-1 consumed: shift the window to start at k
                        const int sh = k - k0;          // 1..3 (selects: no indexed registers)
                        const unsigned long long t1 = u[1], t2 = u[2], t3 = u[3];
                        u[0] = sh == 1 ? t1 : sh == 2 ? t2 : t3;
                        u[1] = sh == 1 ? t2 : sh == 2 ? t3 : kSentinel;
                        u[2] = sh == 1 ? t3 : kSentinel;
                        u[3] = kSentinel;
                        ub = k;
                    }
                }
                if (k == k1) {
                    st_agent(xu + r, (unsigned long long)__double_as_longlong(fm ? acc : y ? acc * dr : acc / dr));
                    pending = false;
                }
            }
            if (__any(pending)) {
                __builtin_amdgcn_s_sleep(GG_FLOW_SLEEP);
                if (++spins > kSpinLimit) {
                    if (pending) atomicOr(err, 1);
                    pending = false;
                }
            }
        }
    }
}

// Bordered grid, forward solve (DevTri::tail): a grid row's tail terms lead
// its canonical order, so b[row] - (its tail terms, in order) is exactly the
// head of the row's own sum; it is formed here, in place, once the tail is
// solved, and the wavefront continues the sum from it.  One row per thread.
__global__ void k_border_sub(Gate g, int nrow, const long long *__restrict__ slot, const int *__restrict__ rp,
                             const int *__restrict__ ci, const double *__restrict__ v,
                             const double *__restrict__ x, double *b, int fm)
{
    if (gated(g)) return;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nrow) return;
    const long long p = slot[q];
    double acc = b[p];
    // fm: GG_DIV_FMA's unit L rows (the tail terms lead the fused row too)
    for (int k = rp[q]; k < rp[q + 1]; k++) acc = fm ? __builtin_fma(-v[k], x[ci[k]], acc) : acc - v[k] * x[ci[k]];
    b[p] = acc;
}

// A small bordered-grid tail (DevTri::tail_small) in ONE workgroup: its level
// sets one after the other with a barrier between (no sentinel pre-fill, no
// polls), each row with k_trsv_level's operations (fm: GG_DIV_FMA's rows, y:
// the multiply); then, for the forward solve, the mesh rows' tail terms
// (k_border_sub's operations) -- the three or four launches of the general
// path (fill, flow, coupling) in one: 4-5 us each for an 800-row tail
__global__ __launch_bounds__(1024) void k_tail_small(Gate g, int nlev, const int *__restrict__ lev_ptr,
                                                     const int *__restrict__ rows, const int *__restrict__ rp,
                                                     const int *__restrict__ ci, const double *__restrict__ v,
                                                     const double *__restrict__ d, const double *__restrict__ y,
                                                     int fm, const double *b, double *x, int ncoup,
                                                     const long long *__restrict__ cslot, const int *__restrict__ crp,
                                                     const int *__restrict__ cci, const double *__restrict__ cv,
                                                     double *bmut, int cfm)
{
    if (gated(g)) return;
    for (int l = 0; l < nlev; l++) {
        const int q1 = lev_ptr[l + 1];
        for (int q = lev_ptr[l] + (int)threadIdx.x; q < q1; q += (int)blockDim.x) {
            const int r = rows[q];
            double acc;
            if (fm) {
                acc = y ? b[r] * y[r] : b[r];
                for (int k = rp[r]; k < rp[r + 1]; k++) acc = __builtin_fma(-v[k], x[ci[k]], acc);
            } else {
                acc = b[r];
                for (int k = rp[r]; k < rp[r + 1]; k++) acc = acc - v[k] * x[ci[k]];
                acc = y ? acc * y[r] : acc / d[r];
            }
            x[r] = acc;
        }
        __syncthreads();
    }
    for (int q = threadIdx.x; q < ncoup; q += blockDim.x) {
        const long long p = cslot[q];
        double acc = bmut[p];
        for (int k = crp[q]; k < crp[q + 1]; k++)
            acc = cfm ? __builtin_fma(-cv[k], x[cci[k]], acc) : acc - cv[k] * x[cci[k]];
        bmut[p] = acc;
    }
}

// The sharded solve's separator step in ONE launch (dd.hip apply_minv): the
// three row phases of SepFlow -- separator L rows (b_S - L_SI y_I, then the
// separator triangle's terms, / d), separator U rows (y_S, then the triangle's
// terms, / d), interface rows of the interior (y_I - U_IS x_S, in place) -- as
// one dataflow task list in that order (each phase in level order), short rows
// one per lane as in k_trsv_flow.  Every row runs the operations and order of
// the launches it replaces (k_sub_seq, k_trsv_flow, k_trsv_flow, k_sub_seq),
// so the result is the same bit for bit.  Values a row polls: its own-phase
// sources (sentinel = not ready) and, in the U phase, b = y_S.
__global__ __launch_bounds__(kBlock) void k_sep_flow(Gate g, int ntask, const int4 *__restrict__ tasks,
                                                     const int *__restrict__ rows, SepFlow f, int *err)
{
    if (gated(g)) return;
    const int lane = threadIdx.x & 63;
    const long long wid = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
    const long long nw = (gridDim.x * (long long)blockDim.x) >> 6;
    for (long long t = wid; t < ntask; t += nw) {
        const int4 tk = tasks[t];
        const SepPhase &P = f.ph[tk.z];
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(P.src);
        const int r = lane < tk.y ? rows[tk.x + lane] : -1;
        bool pending = r >= 0;
        int k = pending ? P.rp[r] : 0;
        const int k1 = pending ? P.rp[r + 1] : 0;
        double acc = 0.0;
        bool have_b = !pending;
        if (pending && !P.bpoll) {
            acc = P.b[r];
            if (P.prp)
                for (int q = P.prp[r]; q < P.prp[r + 1]; q++) acc -= P.pv[q] * P.px[P.pci[q]];
            have_b = true;
        }
        int spins = 0;
        while (__any(pending)) {
            if (pending && !have_b) {
                const unsigned long long u = ld_agent(reinterpret_cast<const unsigned long long *>(P.b) + r);
                if (u != kSentinel) {
                    acc = __longlong_as_double((long long)u);
                    have_b = true;
                }
            }
            if (pending && have_b) {
                bool stop = false;
                while (!stop && k < k1) {
                    unsigned long long u[4];            // up to 4 polls in flight
#pragma unroll
                    for (int j = 0; j < 4; j++) u[j] = k + j < k1 ? ld_agent(src + P.ci[k + j]) : 0ull;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (stop || k >= k1) break;
                        if (u[j] == kSentinel) { stop = true; break; }
                        acc = acc - P.v[k] * __longlong_as_double((long long)u[j]);
                        k++;
                    }
                }
                if (k == k1) {
                    const double o = P.d ? acc / P.d[r] : acc;
                    st_agent(reinterpret_cast<unsigned long long *>(P.x) + r, (unsigned long long)__double_as_longlong(o));
                    pending = false;
                }
            }
            if (__any(pending)) {
                __builtin_amdgcn_s_sleep(4);
                if (++spins > kSpinLimit) {
                    if (pending) atomicOr(err, 1);
                    pending = false;
                }
            }
        }
    }
}

// ================================================ ILU(0) factorization (device)
// leftILU's column elimination (src/leftILU.cu:27-336: cpuSequentialTriSolve
// :769-825 per column, columns in generateLevel :339-368 order) as a dataflow
// kernel.  Lane = column c; a wave takes 64 consecutive columns, the grid
// strides over the columns in ascending order (all blocks co-resident, so the
// smallest unfinished column can always progress).  Per column:
//  1. its level: max(level[r] + 1) over the rows r < c of its U part whose
//     ORIGINAL value is not |a| < 1e-9 (generateLevel), published in level[c];
//  2. the serial order of the reference processes columns by (level, index),
//     so a source column r < c (a U-part row of c) was finished before c iff
//     level[r] <= level[c]: then wait for done[r] and read r's factored
//     values, otherwise read r's ORIGINAL values (r had not been processed);
//  3. the column update in the reference's order (ascending U-part rows, then
//     the L part divided by the diagonal, 0 when |diag| < 1e-9), written with
//     agent-scope stores, drained, then done[c] published.
// Lanes of one wave can depend on each other, so every lane retries inside a
// wave-uniform loop instead of spinning alone.  Spins are bounded (err bit 0).
__device__ __forceinline__ bool ilu_zero(double a) { return __builtin_fabs(a) < 1e-9; }   // Equal(a, 0)

__global__ __launch_bounds__(kBlock) void k_ilu0_columns(int n, const int *__restrict__ cp,
                                                         const int *__restrict__ ri,
                                                         const double *__restrict__ cv0, double *cv,
                                                         int *level, int *done, int *err)
{
    const int lane = threadIdx.x & 63;
    const long long wid = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
    const long long nw = (gridDim.x * (long long)blockDim.x) >> 6;
    for (long long base = wid * 64; base < n; base += nw * 64) {
        const int c = (int)(base + lane);
        int state = c < n ? 0 : 2;             // 0: level, 1: factor, 2: finished
        int lev = 0;
        int spins = 0;
        const int lb = c < n ? cp[c] : 0, ub = c < n ? cp[c + 1] : 0;
        while (__any(state != 2)) {
            bool moved = false;
            if (state == 0) {
                bool ready = true;
                int l = 0;
                for (int k = lb; k < ub; k++) {
                    const int r = ri[k];
                    if (r >= c) break;
                    const int lr = ld_agent_i(level + r);
                    if (lr < 0) { ready = false; break; }
                    if (!ilu_zero(cv0[k]) && lr + 1 > l) l = lr + 1;
                }
                if (ready) {
                    lev = l;
                    st_agent_i(level + c, l);
                    state = 1;
                    moved = true;
                }
            }
            if (state == 1) {
                bool ready = true;
                for (int k = lb; k < ub; k++) {
                    const int r = ri[k];
                    if (r >= c) break;
                    if (ld_agent_i(level + r) <= lev && ld_agent_i(done + r) == 0) { ready = false; break; }
                }
                if (ready) {
                    double u_diag = 0.0;
                    for (int k = lb; k < ub - 1; k++) {
                        const int cr = ri[k];
                        if (cr > c) break;
                        if (cr == c) { u_diag = ld_agent_d(cv + k); break; }
                        const bool fin = ld_agent_i(level + cr) <= lev;
                        int q = cp[cr];
                        const int qe = cp[cr + 1];
                        const double ukt = ld_agent_d(cv + k);
                        for (int p = k + 1; p < ub; p++) {
                            const int r2 = ri[p];
                            while (q < qe && ri[q] < r2) q++;
                            if (q == qe) break;
                            if (ri[q] == r2) {
                                const double lq = fin ? ld_agent_d(cv + q) : cv0[q];
                                st_agent_d(cv + p, ld_agent_d(cv + p) - lq * ukt);
                            }
                        }
                    }
                    for (int k = lb; k < ub; k++) {
                        if (ri[k] <= c) continue;
                        st_agent_d(cv + k, ilu_zero(u_diag) ? 0.0 : ld_agent_d(cv + k) / u_diag);
                    }
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // values out before the flag
                    st_agent_i(done + c, 1);
                    state = 2;
                    moved = true;
                }
            }
            if (!moved && state != 2) {
                __builtin_amdgcn_s_sleep(2);
                if (++spins > kSpinLimit) {
                    atomicOr(err, 1);
                    state = 2;
                }
            }
        }
    }
}

// ILU(k) numeric factorization (ilukC, src/iluk.cpp:108-188) on lofC's pattern
// (host, iluk_pattern): row i = prow[i] .. prow[i+1], every row ascending (its
// nl[i] L entries, the diagonal, its U part).  One WAVE per row; a row's pivots
// (its L entries) are taken one after the other in ascending column order --
// the order ilukC applies them, so every entry sees the same updates in the
// same order and the factors are bit-identical:
//   wait done[k]; l = val[t] * Dinv[k]; for the U entries (k, c) of row k, in
//   parallel over the lanes: if c is in row i's pattern, val[i, c] -= l * u
// then Dinv[i] = 1 / val[diag] (err bit 2 on a zero pivot, src/iluk.cpp:175-185),
// the row's values stored write-through, drained, done[i] published.
// Ordinary rows (<= kIlukCap entries) are staged in the wave's LDS (columns
// and values; a column is found by binary search above the pivot's position);
// longer rows (the hub rows of circuit matrices) keep their values in HBM and
// find columns through a dense column -> position map of their own (scratch,
// n ints per long-row wave, -1 outside the row).  Rows are split into the two
// lists (ascending); the first `long_blocks` blocks take the long list, the
// rest the short one, each wave its list's rows in ascending order: with every
// block co-resident the smallest unfinished row always progresses.  Spins are
// bounded (err bit 0).
constexpr int kIlukCap = 3200;
__device__ __forceinline__ int lds_bsearch(const int *a, int lo, int hi, int c)
{
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && a[lo] == c) ? lo : -1;
}

__global__ __launch_bounds__(kBlock) void k_iluk_wave(int n, const long long *__restrict__ prow,
                                                      const int *__restrict__ nl,
                                                      const int *__restrict__ pcol, double *val,
                                                      double *dinv, int *done,
                                                      const int *__restrict__ rows_short, int nshort,
                                                      const int *__restrict__ rows_long, int nlong,
                                                      int long_blocks, int *scratch, int *err)
{
    __shared__ int scol[kBlock / 64][kIlukCap];
    __shared__ double sval[kBlock / 64][kIlukCap];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool lng = (int)blockIdx.x < long_blocks;
    const int gw = (lng ? (int)blockIdx.x : (int)blockIdx.x - long_blocks) * (kBlock / 64) + w;
    const int nw = (lng ? long_blocks : (int)gridDim.x - long_blocks) * (kBlock / 64);
    const int cnt = lng ? nlong : nshort;
    const int *rows = lng ? rows_long : rows_short;
    int *jw = lng ? scratch + (long long)gw * n : nullptr;
    int *sc = scol[w];
    double *sv = sval[w];
    bool dead = false;
    for (int q = gw; q < cnt && !dead; q += nw) {
        const int i = rows[q];
        const long long p0 = prow[i];
        const int len = (int)(prow[i + 1] - p0), nli = nl[i];
        if (!lng) {
            for (int t = lane; t < len; t += 64) {
                sc[t] = pcol[p0 + t];
                sv[t] = val[p0 + t];
            }
        } else {
            for (int t = lane; t < len; t += 64) __hip_atomic_store(jw + pcol[p0 + t], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        for (int j = 0; j < nli && !dead; j++) {
            const int k = lng ? pcol[p0 + j] : sc[j];
            int spins = 0;
            while (__builtin_amdgcn_readfirstlane(ld_agent_i(done + k)) == 0) {
                __builtin_amdgcn_s_sleep(2);
                if (++spins > kSpinLimit) {
                    if (lane == 0) atomicOr(err, 1);
                    dead = true;
                    break;
                }
            }
            const double l = (lng ? ld_agent_d(val + p0 + j) : sv[j]) * ld_agent_d(dinv + k);
            if (lane == 0) {
                if (lng) st_agent_d(val + p0 + j, l);
                else sv[j] = l;
            }
            const long long u0 = prow[k] + nl[k] + 1, u1 = prow[k + 1];
            for (long long e = u0 + lane; e < u1; e += 64) {
                const int c = pcol[e];
                const double u = ld_agent_d(val + e);
                if (lng) {
                    const int pos = __hip_atomic_load(jw + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (pos >= 0) st_agent_d(val + p0 + pos, ld_agent_d(val + p0 + pos) - l * u);
                } else {
                    const int pos = lds_bsearch(sc, j + 1, len, c);
                    if (pos >= 0) sv[pos] = sv[pos] - l * u;
                }
            }
            if (lng) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const double dg = lng ? ld_agent_d(val + p0 + nli) : sv[nli];
        if (!lng)
            for (int t = lane; t < len; t += 64) st_agent_d(val + p0 + t, sv[t]);
        if (lane == 0) {
            if (dg == 0.0) atomicOr(err, 2);
            st_agent_d(dinv + i, 1.0 / dg);
        }
        if (lng)
            for (int t = lane; t < len; t += 64) __hip_atomic_store(jw + pcol[p0 + t], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the row's values out before the flag
        if (lane == 0) st_agent_i(done + i, 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // LDS reads done before the next row's staging
    }
}

// A's values into the ILU(k) pattern (val pre-zeroed), ilukC's initial
// scatter (src/iluk.cpp:120-133): one thread per row, entries in CSR order (a
// repeated column keeps its last value, as the reference's assignment does),
// each position found by binary search in the row's ascending columns
__global__ __launch_bounds__(kBlock) void k_iluk_scatter(int n, const int *__restrict__ arp,
                                                         const int *__restrict__ aci,
                                                         const double *__restrict__ av,
                                                         const long long *__restrict__ prow,
                                                         const int *__restrict__ pcol, double *val)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const long long p0 = prow[i], p1 = prow[i + 1];
        for (int e = arp[i]; e < arp[i + 1]; e++) {
            const int c = aci[e];
            long long lo = p0, hi = p1;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (pcol[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            val[lo] = av[e];                     // every entry of A is in its row's pattern
        }
    }
}

// ================================================== transient step (C5)
// PULSE source values at time index it (gen_PULSEut_kernel, src/kernels.cu:223-245);
// pulse[k] = {vlo, vhi, td, tr, tf, tw, tp}
// Source values at time index it, t = it * h (mytime = idxt * tstep), one
// thread per source, kind[k] / data[dptr[k] .. dptr[k+1]):
//   GG_SRC_DC     {value}                              gen_dcVt_kernel   src/kernels.cu:73-85
//   GG_SRC_PULSE  {vlo, vhi, td, tr, tf, tw, tp}       gen_PULSEut_kernel src/kernels.cu:223-245
//   GG_SRC_PWL    {t0, v0, t1, v1, ...}                gen_PWLut_kernel  src/kernels.cu:146-176
// (PWL before t0: v0; the reference reads v[-1] there)
__device__ __forceinline__ double pulse_value(const double *q, double t)
{
    const double vlo = q[0], vhi = q[1], td = q[2], tr = q[3], tf = q[4], tw = q[5], tp = q[6];
    t = t - floor(t / tp) * tp;
    if (t < td) return vlo;
    if (t < td + tr) return vlo + (t - td) * (vhi - vlo) / tr;
    if (t < td + tr + tw) return vhi;
    if (t < td + tr + tw + tf) return vhi - (t - td - tr - tw) * (vhi - vlo) / tf;
    return vlo;
}
__device__ __forceinline__ double pwl_value(const double *tv, int np, double t)
{
    if (np <= 0) return 0.0;
    double value = tv[1];
    int i;
    for (i = 0; i < np; i++) {
        if (t < tv[2 * i]) {
            if (i > 0)
                value = tv[2 * i + 1] - (tv[2 * i] - t) * (tv[2 * i + 1] - tv[2 * i - 1]) /
                                            (tv[2 * i] - tv[2 * i - 2]);
            break;
        }
    }
    if (i == np) value = tv[2 * np - 1];
    return value;
}
__global__ void k_sources(int nsrc, const int *kind, const int *dptr, const double *data, int it, double h,
                          double *u)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nsrc) return;
    const double *q = data + dptr[k];
    const double t = it * h;
    double value = 0.0;
    if (kind[k] == GG_SRC_DC) value = q[0];
    else if (kind[k] == GG_SRC_PULSE) value = pulse_value(q, t);
    else value = pwl_value(q, (dptr[k + 1] - dptr[k]) / 2, t);
    u[k] = value;
}

// w = B u + (C/h) x_prev as the reference step driver forms it
// (src/mna_solve_gpu_gmres.cpp:585-591): w = 0; w += B u (cs_dl_gaxpy, sources
// of a row in column order); xnr = 0; xnr += (C/h) x; w += xnr.  B is an
// incidence matrix (+1 per source), C/h diagonal.
__global__ void k_transient_rhs(int n, const int *src_ptr, const int *src_idx, const double *u,
                                const double *cdiag, const double *x, double *w)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    double bu = 0.0;
    for (int q = src_ptr[r]; q < src_ptr[r + 1]; q++) bu = bu + 1.0 * u[src_idx[q]];
    double xnr = 0.0;
    xnr = xnr + cdiag[r] * x[r];
    w[r] = bu + xnr;
}

// w = B u + R x_prev for a general MNA system (gg_transient_mna, the
// wrapperGMRESforPG path): B (n x nsrc) and R = C/h (n x n, capacitor stamps
// between nodes included) in CSR.  cs_dl_gaxpy (y += A x, column by column)
// accumulates each row in ascending column order from 0.0, which is the CSR
// row order here: bu = B u, xnr = R x, w = bu + xnr (the driver's w += xnr).
__global__ void k_transient_rhs_csr(int n, const int *bp, const int *bi, const double *bv, const double *u,
                                    const int *rp, const int *ri, const double *rv, const double *x,
                                    double *w)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    double bu = 0.0;
    for (int q = bp[r]; q < bp[r + 1]; q++) bu = bu + bv[q] * u[bi[q]];
    double xnr = 0.0;
    for (int q = rp[r]; q < rp[r + 1]; q++) xnr = xnr + rv[q] * x[ri[q]];
    w[r] = bu + xnr;
}

// tap-node voltage statistics of the transient run (the ir_info block of the
// step driver, src/mna_solve_gpu_gmres.cpp:285-292, 633-645, 780-797): max,
// min and the running sum, seeded with the initial state; avg = sum / time
// points, IR = max - min at the end
__global__ void k_taps(int ntap, const int *tap, const double *x, double *mx, double *mn, double *sm, int mode,
                       double npts)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ntap) return;
    if (mode == 2) {                       // finish: sum -> avg (IR = max - min on the host)
        sm[j] = sm[j] / npts;
        return;
    }
    const double v = x[tap[j]];
    if (mode == 0) {
        mx[j] = v;
        mn[j] = v;
        sm[j] = v;
        return;
    }
    if (mx[j] < v) mx[j] = v;
    if (v < mn[j]) mn[j] = v;
    sm[j] += v;
}

__global__ void k_gather_ports(int nport, const int *port, const double *x, double *out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nport) out[j] = x[port[j]];
}

// ---- batched (many-RHS) helpers: blockIdx.y = scenario ----------------------
// out_sc[i] = idx[i] < 0 ? 0 : in_sc[idx[i]], in / out strides zin / zout bytes
__global__ void k_gather_b(const double *in, long long zin, const long long *idx, double *out, long long zout,
                           long long n)
{
    in = zp(in, zin, blockIdx.y);
    out = zp(out, zout, blockIdx.y);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        const long long s = idx[i];
        out[i] = s < 0 ? 0.0 : in[s];
    }
}
// every scenario's control block at the start of a solve (as the host writes
// the single solver's)
__global__ void k_init_state_b(DevState *ds, long long zs, int nsc, double tol, int max_iter, int m)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nsc) return;
    DevState h{};
    h.tol = tol;
    h.max_iter = max_iter;
    h.m = m;
    h.j = 1;
    *zp(ds, zs, q) = h;
}
// the scenarios' control blocks (DevState, CgState, BiState) side by side in a read-back
// slot, and behind them the error word after every launch before this one
// (batch_common.h ReadRing: one copy to the host per chunk)
template <class State>
__global__ void k_pack_states_b(const State *st0, long long zs, int nsc, State *out, const int *err)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nsc) out[q] = *zp(st0, zs, q);
    if (q == nsc) *reinterpret_cast<int *>(out + nsc) = *err;
}
// transient step of every scenario: u_sc = its sources at time index it; w_sc
// = B_sc u_sc + (C/h) x_sc (k_sources + k_transient_rhs per scenario; tables
// concatenated, scenario sc's sources [soff[sc], soff[sc+1]) and its B^T rows
// at sptr + sc * (n + 1); x and w natural order, stride ldx doubles)
__global__ void k_sources_b(const int *soff, const int *kind, const int *dptr, const double *data, int it,
                            double h, double *u)
{
    const int q = blockIdx.y;
    const int k = soff[q] + blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= soff[q + 1]) return;
    const double *d = data + dptr[k];
    const double t = it * h;
    double value = 0.0;
    if (kind[k] == GG_SRC_DC) value = d[0];
    else if (kind[k] == GG_SRC_PULSE) value = pulse_value(d, t);
    else value = pwl_value(d, (dptr[k + 1] - dptr[k]) / 2, t);
    u[k] = value;
}
__global__ void k_transient_rhs_b(int n, const int *sptr, const int *sidx, const double *u, const double *cdiag,
                                  const double *x, double *w, long long ldx)
{
    const int q = blockIdx.y;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int *sp = sptr + (long long)q * (n + 1);
    double bu = 0.0;
    for (int k = sp[r]; k < sp[r + 1]; k++) bu = bu + 1.0 * u[sidx[k]];
    double xnr = 0.0;
    xnr = xnr + cdiag[r] * x[(long long)q * ldx + r];
    w[(long long)q * ldx + r] = bu + xnr;
}
__global__ void k_gather_ports_b(int nport, const int *port, const double *x, long long ldx, double *out,
                                 long long ldo)
{
    const int q = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nport) out[(long long)q * ldo + j] = x[(long long)q * ldx + port[j]];
}

// ============================================================ GMRES kernels
__global__ void k_set_normb(const double *part, int G, DevState *ds, long long zs = 0)
{
    part = zp(part, zs, blockIdx.y);
    ds = zp(ds, zs, blockIdx.y);
    double s = sum_partials(part, G);
    if (threadIdx.x == 0) {
        double nb = sqrt(s);
        ds->normb = (nb == 0.0) ? 1.0 : nb;     // src/gmres.cu:604
    }
}

__global__ void k_init_beta(const double *part, int G, DevState *ds, double *hist, long long zs = 0)
{
    part = zp(part, zs, blockIdx.y);
    ds = zp(ds, zs, blockIdx.y);
    hist = zp(hist, zs, blockIdx.y);
    double s = sum_partials(part, G);
    if (threadIdx.x == 0) {
        double beta = sqrt(s);
        double resid = beta / ds->normb;
        ds->beta = beta;
        ds->resid = resid;
        hist[0] = resid;
        ds->hist_len = 1;
        ds->j = 1;
        if (resid <= ds->tol) ds->done = DONE_INIT;   // "<=" (src/gmres.cu:608)
    }
}

// v0 = r * (1/beta); s = 0; s[0] = beta; nit = min(m, max_iter - j + 1)
__global__ __launch_bounds__(kBlock) void k_init_cycle(DevState *ds, const double *r, double *v0,
                                                       double *s, long long units, long long zs = 0)
{
    ds = zp(ds, zs, blockIdx.y);
    r = zp(r, zs, blockIdx.y);
    v0 = zp(v0, zs, blockIdx.y);
    s = zp(s, zs, blockIdx.y);
    if (ds->done) return;
    if (ds->max_iter - ds->j + 1 <= 0) {   // a cycle past max_iter (pipelined): nothing runs
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            ds->nit = 0;
            ds->done |= DONE_EXH;
        }
        return;
    }
    const double beta = ds->beta;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int nit = ds->max_iter - ds->j + 1;
        if (nit > ds->m) nit = ds->m;
        ds->nit = nit;
        for (int k = 0; k <= ds->m; k++) s[k] = 0.0;
        s[0] = beta;
    }
    const double inv = 1.0 / beta;
    for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units;
         u += (long long)gridDim.x * kBlock) {
        double2 a = ld2(r, u);
        a.x = inv * a.x;
        a.y = inv * a.y;
        st2(v0, u, a);
    }
}

// One MGS step k of inner iteration i (src/gmres.cu:638-641):
//   h = <w, v_k> (from the previous kernel's partials); H[k,i] = h;
//   w = (-h) v_k + w;  partials of <w, vnext>  (vnext = v_{k+1}, or w for the norm)
// Each thread owns units u = g*256 + t + j*G*256 (j = 0, 1, ...), accumulated in
// ascending j (the oracle's blocked dot order); kUnroll of them are loaded
// before any is used so a thread keeps several 16-B loads per stream in flight.

template <bool NORM>
__global__ __launch_bounds__(kBlock) void k_mgs_step(Gate g, int i, int k, int m,
                                                     double *__restrict__ w,
                                                     const double *__restrict__ vk,
                                                     const double *__restrict__ vnext,
                                                     const double *part_in, double *part_out,
                                                     double *H, int G, long long units,
                                                     long long dunits, long long zs = 0)
{
    // the AXPY runs over [0, units); the next dot accumulates over [0, dunits)
    // (dunits < units on the shards of a sharded solve that do not own the
    // separator replica); part_in holds G partials (all shards' in that case)
    if (gated_z(g, zs, blockIdx.y)) return;
    if (zs) {
        const int sc = blockIdx.y;
        w = zp(w, zs, sc);
        vk = zp(vk, zs, sc);
        vnext = zp(vnext, zs, sc);
        part_in = zp(part_in, zs, sc);
        part_out = zp(part_out, zs, sc);
        H = zp(H, zs, sc);
    }
    double acc = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x;
    double2 wv[kUnroll], vv[kUnroll], nv[kUnroll];
    auto load = [&]() {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                wv[j] = ld2(w, u);          // w: re-read every step, kept in the caches
                vv[j] = ld2_nt(vk, u);      // the basis vectors are streamed
                if (!NORM) nv[j] = ld2_nt(vnext, u);
            }
        }
    };
    load();                 // the first chunk is in flight while h is summed
    const double h = sum_partials(part_in, G);
    if (blockIdx.x == 0 && threadIdx.x == 0) H[k + i * (m + 1)] = h;
    const double a = -h;
    while (u0 < units) {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                wv[j].x = a * vv[j].x + wv[j].x;
                wv[j].y = a * vv[j].y + wv[j].y;
                st2(w, u, wv[j]);
                if (NORM) nv[j] = wv[j];
                if (u < dunits) {
                    acc += wv[j].x * nv[j].x;
                    acc += wv[j].y * nv[j].y;
                }
            }
        }
        u0 += kUnroll * stride;
        load();
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) part_out[blockIdx.x] = acc;
}

// ---- CGS2 (the sharded solve's GG_SOLVE_CGS2): classical Gram-Schmidt with
// one re-orthogonalization, h = V^T w; w -= V h; h2 = V^T w; w -= V h2;
// H[:, i] = h + h2 -- three all-gathers per inner iteration (h, h2, ||w||)
// instead of MGS's i + 2.  Every dot keeps k_dot's tree (thread t of block b:
// units b*256 + t + j*G*256 ascending, block_sum), so the oracle restates it
// bit for bit (orc_set_orth).
__global__ __launch_bounds__(kBlock) void k_multidot(Gate g, const double *__restrict__ w,
                                                     const double *__restrict__ V, long long ldv, int nk,
                                                     double *part, int G, long long dunits)
{
    // part[k*G + blockIdx.x] = block partial of <w, v_k>, k = blockIdx.y*kCgsKC + kk < nk
    if (gated(g)) return;
    const int k0 = blockIdx.y * kCgsKC;
    const int kc = nk - k0 < kCgsKC ? nk - k0 : kCgsKC;
    double acc[kCgsKC];
#pragma unroll
    for (int kk = 0; kk < kCgsKC; kk++) acc[kk] = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < dunits; u += stride) {
        const double2 a = ld2(w, u);
#pragma unroll
        for (int kk = 0; kk < kCgsKC; kk++) {
            if (kk < kc) {
                const double2 b = ld2_nt(V + (long long)(k0 + kk) * ldv, u);
                acc[kk] += a.x * b.x;
                acc[kk] += a.y * b.y;
            }
        }
    }
    block_sum_store<kCgsKC>(acc, kc, part + (long long)k0 * G + blockIdx.x, G);
}
// h[k] = sum of every shard's partials of dot k (shard q's at part + q*cnt + k*G,
// summed in sum_partials' order over the P*G partials, shard-major);
// add = 0: H[k, i] = h[k]; add = 1: H[k, i] += h[k].  One block per k.
__global__ __launch_bounds__(kBlock) void k_cgs_reduce(Gate g, const double *part, int P, int G, long long cnt,
                                                       double *h, double *H, int i, int m, int add)
{
    if (gated(g)) return;
    const int k = blockIdx.x;
    double v = 0.0;
    for (int e = threadIdx.x; e < P * G; e += kBlock) v += part[(long long)(e / G) * cnt + (long long)k * G + e % G];
    v = block_sum(v);
    if (threadIdx.x == 0) {
        h[k] = v;
        double *hk = H + k + (long long)i * (m + 1);
        *hk = add ? *hk + v : v;
    }
}
// a = a - sum_k h[k] v_k(u), k ascending (a = (-h_k) v_k + a, the MGS AXPY's
// rounding), the loads of up to kCgsChunk v_k issued before their
// multiply-adds (a thread owns one or a few units: one load round trip per
// chunk, not per vector); the chunk's values are left in b for the caller.
constexpr int kCgsChunk = 32;
__device__ __forceinline__ void cgs_axpy_chunk(double2 &a, double2 (&b)[kCgsChunk], const double *__restrict__ V,
                                               long long ldv, const double *h, int k0, int nk, long long u)
{
#pragma unroll
    for (int kk = 0; kk < kCgsChunk; kk++)
        if (k0 + kk < nk) b[kk] = ld2_nt(V + (long long)(k0 + kk) * ldv, u);
#pragma unroll
    for (int kk = 0; kk < kCgsChunk; kk++) {
        if (k0 + kk < nk) {
            const double c = -h[k0 + kk];
            a.x = c * b[kk].x + a.x;
            a.y = c * b[kk].y + a.y;
        }
    }
}
// w = w - sum_k h[k] v_k (per element, k ascending: w = (-h_k) v_k + w as the
// MGS AXPY); norm: block partials of <w, w> over [0, dunits) into part_norm
template <bool NORM>
__global__ __launch_bounds__(kBlock) void k_cgs_update(Gate g, double *__restrict__ w,
                                                       const double *__restrict__ V, long long ldv,
                                                       const double *h, int nk, long long units,
                                                       long long dunits, double *part_norm)
{
    if (gated(g)) return;
    double acc = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units; u += stride) {
        double2 a = ld2(w, u);
        double2 b[kCgsChunk];
        for (int k0 = 0; k0 < nk; k0 += kCgsChunk) cgs_axpy_chunk(a, b, V, ldv, h, k0, nk, u);
        st2(w, u, a);
        if (NORM && u < dunits) {
            acc += a.x * a.x;
            acc += a.y * a.y;
        }
    }
    if (NORM) {
        acc = block_sum(acc);
        if (threadIdx.x == 0) part_norm[blockIdx.x] = acc;
    }
}

// CGS2's first update fused with the second pass's dot partials: w = w - sum_k
// h[k] v_k (as k_cgs_update), then the block partials of <w, v_k>, k < nk, over
// [0, dunits) into part[k*G + block] -- the same unit -> thread assignment and
// accumulation order as k_multidot (G blocks, grid stride), so bit-identical to
// the two launches; each v_k(u) is read once (kept in registers between the
// update and the dots).
constexpr int kCgsFuseMax = kCgsChunk;       // dots held per thread (else two launches)
__global__ __launch_bounds__(kBlock) void k_cgs_update_dot(Gate g, double *__restrict__ w,
                                                           const double *__restrict__ V, long long ldv,
                                                           const double *h, int nk, long long units,
                                                           long long dunits, double *part, int G)
{
    if (gated(g)) return;
    double acc[kCgsFuseMax];
#pragma unroll
    for (int k = 0; k < kCgsFuseMax; k++) acc[k] = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units; u += stride) {
        double2 a = ld2(w, u);
        double2 b[kCgsChunk];
        cgs_axpy_chunk(a, b, V, ldv, h, 0, nk, u);
        st2(w, u, a);
        if (u < dunits) {
#pragma unroll
            for (int k = 0; k < kCgsFuseMax; k++) {
                if (k < nk) {
                    acc[k] += a.x * b[k].x;
                    acc[k] += a.y * b[k].y;
                }
            }
        }
    }
    block_sum_store<kCgsFuseMax>(acc, nk, part + blockIdx.x, G);   // static indices: acc stays in registers
}

// H[i+1,i] = ||w||; Givens on column i; residual check; v_{i+1} = w * (1/H[i+1,i])
__global__ __launch_bounds__(kBlock) void k_arnoldi_finalize(Gate g, int i, int m, DevState *ds,
                                                             const double *part, int G,
                                                             const double *w, double *vnext,
                                                             double *H, double *cs, double *sn,
                                                             double *s, double *hist,
                                                             long long units, long long zs = 0)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    if (zs) {
        const int sc = blockIdx.y;
        ds = zp(ds, zs, sc);
        part = zp(part, zs, sc);
        w = zp(w, zs, sc);
        vnext = zp(vnext, zs, sc);
        H = zp(H, zs, sc);
        cs = zp(cs, zs, sc);
        sn = zp(sn, zs, sc);
        s = zp(s, zs, sc);
        hist = zp(hist, zs, sc);
    }
    const double hn = sqrt(sum_partials(part, G));
    if (blockIdx.x == 0 && threadIdx.x == 0) givens_column(i, hn, H + i * (m + 1), cs, sn, s, hist, ds);
    // lucky breakdown (hn == 0): the reference divides by zero; v_{i+1} := 0
    const double inv = (hn != 0.0) ? 1.0 / hn : 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x; u0 < units; u0 += 4 * stride) {
        double2 a[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (u0 + j * stride < units) a[j] = ld2(w, u0 + j * stride);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (u0 + j * stride < units) {
                a[j].x = inv * a[j].x;
                a[j].y = inv * a[j].y;
                st2(vnext, u0 + j * stride, a[j]);
            }
        }
    }
}

// ---- CGS2 with its exchanges inside the kernels (kernels.h, Xch) ------------
// Four launches per inner iteration instead of nine plus three all-gathers:
// k_multidot_x -> k_cgs_update_x<dots> -> k_cgs_update_x<norm> ->
// k_arnoldi_finalize_x, each producer publishing its block partials into every
// rank's area itself and each consumer reducing them in k_cgs_reduce's order
// (so every value has the bits of the launch-per-step path).  A consumer waits
// only for exchanges its peers' EARLIER launches produce, so the waits form no
// cycle; inside a launch the reducer blocks (blockIdx < nk) hand their values to
// the rest through hx / hf -- they are dispatched first and wait on nothing of
// this launch.  Every spin is bounded (~30 s, err |= 4); after one time-out the
// others give up at once (the broken word hf[kCgsXMax + 1]).
// Memory ordering without cache maintenance: the areas and hx / hf are
// uncached device memory, so a producer's stores are in memory once its
// s_waitcnt has drained them, and a consumer's relaxed system-scope loads
// issued after it saw the flag read memory.  No release / acquire here: on
// gfx950 those write back / invalidate the whole L2 (the first version of this
// path, with them: CGS2 64 -> 278 us per iteration at C2/8).
__device__ __forceinline__ unsigned long long *xk_flag(void *base, int P, long long capd, int src)
{
    return reinterpret_cast<unsigned long long *>(base) + (long long)kMaxShards * kIpcXB + 2LL * P * capd +
           (long long)src * kIpcXF;
}
__device__ __forceinline__ double *xk_slot(void *base, int P, long long capd, unsigned long long seq, int src)
{
    return reinterpret_cast<double *>(base) + (long long)kMaxShards * kIpcXB +
           ((long long)(seq & 1) * P + src) * capd;
}
__device__ __noinline__ bool xk_wait_slow(const unsigned long long *f, unsigned long long seq, const Xch &x)
{
    unsigned long long *broken = x.hf + kCgsXMax + 1;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (unsigned n = 1;; n++) {
        __builtin_amdgcn_s_sleep(1);
        if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= seq) return true;
        if ((n & 255) == 0) {
            if (__hip_atomic_load(broken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) return false;
            if (__builtin_amdgcn_s_memrealtime() - t0 > 3000000000ull) {     // ~30 s of the 100 MHz clock
                atomicOr(x.err, 4);
                __hip_atomic_store(broken, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                return false;
            }
        }
    }
}
__device__ __forceinline__ bool xk_wait(const unsigned long long *f, unsigned long long seq, const Xch &x)
{
    bool ok = true;
    if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < seq) ok = xk_wait_slow(f, seq, x);
    asm volatile("" ::: "memory");        // what follows reads after the flag was seen
    return ok;
}
// thread t < n holds v for index idx of this rank's slot: into the own slot
// and every peer's area, then this block's flag in every peer's area
__device__ __forceinline__ void st_sys(double *p, double v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ double ld_sys(const double *p)
{
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p),
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}
__device__ __forceinline__ void xk_publish(const Xch &x, unsigned long long seq, double *own, bool has,
                                           long long idx, double v, int fblock)
{
    // (loopback: this rank's area stands in for every peer's and receives the
    // values in the slots and flags the peers' would use, q's for peer q)
    if (has) {
        own[idx] = v;
        for (int q = 0; q < x.P; q++)
            if (q != x.me) st_sys(xk_slot(x.pp.base[q], x.P, x.capd, seq, x.loop ? q : x.me) + idx, v);
    }
    __builtin_amdgcn_s_waitcnt(0);          // this thread's stores are in memory
    __syncthreads();
    const int t = threadIdx.x;
    if (t < x.P && t != x.me)
        __hip_atomic_store(xk_flag(x.pp.base[t], x.P, x.capd, x.loop ? t : x.me) + fblock, seq, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}
// dot k over every rank's G block partials, in k_cgs_reduce's order (e = q*G + b,
// thread-strided, block_sum); own = this rank's slot.  A thread takes its
// partials kXkChunk at a time: the chunk's flags polled together (relaxed,
// only the pending ones re-polled), one acquire fence, the chunk's values
// loaded together -- two memory round trips per chunk, not two per partial.
constexpr int kXkChunk = 8;
__device__ __forceinline__ double xk_reduce(const Xch &x, unsigned long long seq, const double *own, int G, int k,
                                           int kfl = 0)
{
    // kfl: the producer's grid took kfl dots per block row (flag (k / kfl) * G + b), 0: one row
    double v = 0.0;
    void *mine = x.pp.base[x.me];
    const int PG = x.P * G;
    const int frow = kfl ? (k / kfl) * G : 0;
    for (int e0 = threadIdx.x; e0 < PG; e0 += kXkChunk * kBlock) {
        unsigned long long f[kXkChunk];
#pragma unroll
        for (int j = 0; j < kXkChunk; j++) {
            const int e = e0 + j * kBlock, q = e / G;
            f[j] = ~0ull;
            if (e < PG && q != x.me)
                f[j] = __hip_atomic_load(xk_flag(mine, x.P, x.capd, q) + frow + e % G, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_SYSTEM);
        }
#pragma unroll
        for (int j = 0; j < kXkChunk; j++) {
            if (f[j] < seq) {
                const int e = e0 + j * kBlock, q = e / G;
                (void)xk_wait(xk_flag(mine, x.P, x.capd, q) + frow + e % G, seq, x);
            }
        }
        __builtin_amdgcn_s_waitcnt(0);
        asm volatile("" ::: "memory");
        double val[kXkChunk];
#pragma unroll
        for (int j = 0; j < kXkChunk; j++) {
            const int e = e0 + j * kBlock, q = e / G, b = e % G;
            const long long idx = (long long)k * G + b;
            val[j] = 0.0;
            if (e < PG)
                val[j] = q == x.me ? own[idx] : ld_sys(xk_slot(mine, x.P, x.capd, seq, q) + idx);
        }
#pragma unroll
        for (int j = 0; j < kXkChunk; j++)
            if (e0 + j * kBlock < PG) v += val[j];
    }
    return block_sum(v);
}
// a reducer's value to every block of the launch (thread 0)
__device__ __forceinline__ void xk_post(const Xch &x, int slot, double v, unsigned long long seq)
{
    st_sys(x.hx + slot, v);
    __builtin_amdgcn_s_waitcnt(0);
    __hip_atomic_store(x.hf + slot, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// block_sum_store's sums, thread k < nk receiving sum k
template <int NK>
__device__ __forceinline__ double block_sum_pick(const double (&acc)[NK], int nk)
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
    const int k = threadIdx.x < nk ? threadIdx.x : 0;
    return (sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k]);
}

__global__ __launch_bounds__(kBlock) void k_multidot_x(Gate g, const double *__restrict__ w,
                                                       const double *__restrict__ V, long long ldv, int nk,
                                                       double *part, int G, long long dunits, Xch x,
                                                       unsigned long long seq)
{
    // block (b, y): dots y*kCgsKC + kk as k_multidot; flag y*G + b
    if (gated(g)) return;
    const int k0 = blockIdx.y * kCgsKC;
    const int kc = nk - k0 < kCgsKC ? nk - k0 : kCgsKC;
    double acc[kCgsKC];
#pragma unroll
    for (int kk = 0; kk < kCgsKC; kk++) acc[kk] = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < dunits; u += stride) {
        const double2 a = ld2(w, u);
#pragma unroll
        for (int kk = 0; kk < kCgsKC; kk++) {
            if (kk < kc) {
                const double2 b = ld2_nt(V + (long long)(k0 + kk) * ldv, u);
                acc[kk] += a.x * b.x;
                acc[kk] += a.y * b.y;
            }
        }
    }
    const double v = block_sum_pick<kCgsKC>(acc, kc);
    xk_publish(x, seq, part, threadIdx.x < kc, (long long)(k0 + threadIdx.x) * G + blockIdx.x, v,
               blockIdx.y * gridDim.x + blockIdx.x);
}

// h = reduced exchange sin (H[k, i] = h, or += with add); w -= V h; then
// DOTS: the partials of <w, v_k> (k_cgs_update_dot), else the norm's
// (k_cgs_update<true>), published as exchange sout into part_out
template <bool DOTS>
__global__ __launch_bounds__(kBlock) void k_cgs_update_x(Gate g, double *__restrict__ w,
                                                         const double *__restrict__ V, long long ldv, int nk,
                                                         long long units, long long dunits, int G,
                                                         const double *part_in, unsigned long long sin, double *H,
                                                         int i, int m, int add, double *part_out, Xch x,
                                                         unsigned long long sout, int kfl)
{
    if (gated(g)) return;
    __shared__ double hs[kCgsXMax];
    for (int k = blockIdx.x; k < nk; k += gridDim.x) {
        const double v = xk_reduce(x, sin, part_in, G, k, kfl);
        if (threadIdx.x == 0) {
            double *hk = H + k + (long long)i * (m + 1);
            *hk = add ? *hk + v : v;
            xk_post(x, k, v, sin);
        }
    }
    if (threadIdx.x < nk) {
        (void)xk_wait(x.hf + threadIdx.x, sin, x);
        hs[threadIdx.x] = ld_sys(x.hx + threadIdx.x);
    }
    __syncthreads();
    double acc[DOTS ? kCgsXMax : 1];
#pragma unroll
    for (int k = 0; k < (DOTS ? kCgsXMax : 1); k++) acc[k] = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units; u += stride) {
        double2 a = ld2(w, u);
        double2 b[kCgsChunk];
        cgs_axpy_chunk(a, b, V, ldv, hs, 0, nk, u);
        st2(w, u, a);
        if (u < dunits) {
            if constexpr (DOTS) {
#pragma unroll
                for (int k = 0; k < kCgsXMax; k++) {
                    if (k < nk) {
                        acc[k] += a.x * b[k].x;
                        acc[k] += a.y * b[k].y;
                    }
                }
            } else {
                acc[0] += a.x * a.x;
                acc[0] += a.y * a.y;
            }
        }
    }
    if constexpr (DOTS) {
        const double v = block_sum_pick<kCgsXMax>(acc, nk);
        xk_publish(x, sout, part_out, threadIdx.x < nk, (long long)threadIdx.x * G + blockIdx.x, v, blockIdx.x);
    } else {
        const double v = block_sum(acc[0]);
        xk_publish(x, sout, part_out, threadIdx.x == 0, blockIdx.x, v, blockIdx.x);
    }
}

// MGS of the sharded solve on the same exchanges (the reference's
// orthogonalization, i + 3 launches per inner iteration instead of 2i + 5):
// k_dot_x = k_dot publishing its partials; k_mgs_step_x = k_mgs_step with h
// reduced from exchange sin by block 0 (sum_partials' order over the P*G
// partials) and its partials published as exchange sout
__global__ __launch_bounds__(kBlock) void k_dot_x(Gate g, const double *a, const double *b, double *part,
                                                  long long units, Xch x, unsigned long long seq)
{
    if (gated(g)) return;
    double acc = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x; u0 < units; u0 += 4 * stride) {
        double2 p[4], q[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const long long u = u0 + j * stride;
            if (u < units) { p[j] = ld2(a, u); q[j] = ld2(b, u); }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (u0 + j * stride < units) {
                acc += p[j].x * q[j].x;
                acc += p[j].y * q[j].y;
            }
        }
    }
    acc = block_sum(acc);
    xk_publish(x, seq, part, threadIdx.x == 0, blockIdx.x, acc, blockIdx.x);
}
template <bool NORM>
__global__ __launch_bounds__(kBlock) void k_mgs_step_x(Gate g, int i, int k, int m, double *__restrict__ w,
                                                       const double *__restrict__ vk,
                                                       const double *__restrict__ vnext, const double *part_in,
                                                       unsigned long long sin, double *part_out, double *H, int G,
                                                       long long units, long long dunits, Xch x,
                                                       unsigned long long sout)
{
    if (gated(g)) return;
    __shared__ double hsh;
    double acc = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x;
    double2 wv[kUnroll], vv[kUnroll], nv[kUnroll];
    auto load = [&]() {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                wv[j] = ld2(w, u);
                vv[j] = ld2_nt(vk, u);
                if (!NORM) nv[j] = ld2_nt(vnext, u);
            }
        }
    };
    load();                 // the first chunk is in flight while h is summed
    if (blockIdx.x == 0) {
        const double v = xk_reduce(x, sin, part_in, G, 0);
        if (threadIdx.x == 0) {
            H[k + i * (m + 1)] = v;
            xk_post(x, 0, v, sin);
        }
    }
    if (threadIdx.x == 0) {
        (void)xk_wait(x.hf, sin, x);
        hsh = ld_sys(x.hx);
    }
    __syncthreads();
    const double a = -hsh;
    while (u0 < units) {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                wv[j].x = a * vv[j].x + wv[j].x;
                wv[j].y = a * vv[j].y + wv[j].y;
                st2(w, u, wv[j]);
                if (NORM) nv[j] = wv[j];
                if (u < dunits) {
                    acc += wv[j].x * nv[j].x;
                    acc += wv[j].y * nv[j].y;
                }
            }
        }
        u0 += kUnroll * stride;
        load();
    }
    acc = block_sum(acc);
    xk_publish(x, sout, part_out, threadIdx.x == 0, blockIdx.x, acc, blockIdx.x);
}

// k_arnoldi_finalize, ||w||^2 reduced from exchange sin by block 0
__global__ __launch_bounds__(kBlock) void k_arnoldi_finalize_x(Gate g, int i, int m, DevState *ds,
                                                               const double *part_in, unsigned long long sin,
                                                               int G, const double *w, double *vnext, double *H,
                                                               double *cs, double *sn, double *s, double *hist,
                                                               long long units, Xch x)
{
    if (gated(g)) return;
    __shared__ double nrm2;
    if (blockIdx.x == 0) {
        const double v = xk_reduce(x, sin, part_in, G, 0);
        if (threadIdx.x == 0) xk_post(x, kCgsXMax, v, sin);
    }
    if (threadIdx.x == 0) {
        (void)xk_wait(x.hf + kCgsXMax, sin, x);
        nrm2 = ld_sys(x.hx + kCgsXMax);
    }
    __syncthreads();
    const double hn = sqrt(nrm2);
    if (blockIdx.x == 0 && threadIdx.x == 0) givens_column(i, hn, H + i * (m + 1), cs, sn, s, hist, ds);
    const double inv = (hn != 0.0) ? 1.0 / hn : 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units; u += stride) {
        double2 a = ld2(w, u);
        a.x = inv * a.x;
        a.y = inv * a.y;
        st2(vnext, u, a);
    }
}

// y = H(0:k,0:k)^-1 s(0:k)  (Update, src/gmres.cu:93-116); k = conv_i or nit-1.
// One wave: lane j keeps y[j] and row j of H in registers; for i = k..0 lane i
// divides, the value is broadcast, lanes j < i subtract -- per element the same
// operations in the same order as the serial back-substitution.
constexpr int kMaxRestart = 64;
__global__ __launch_bounds__(64) void k_update_y(Gate g, int m, DevState *ds, const double *H,
                                                 const double *s, double *y, long long zs = 0)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    ds = zp(ds, zs, blockIdx.y);
    H = zp(H, zs, blockIdx.y);
    s = zp(s, zs, blockIdx.y);
    y = zp(y, zs, blockIdx.y);
    const int lane = threadIdx.x;
    const int k = (ds->done & DONE_INNER) ? ds->conv_i : ds->nit - 1;
    if (lane == 0) ds->upd_k = k;
    const int ld = m + 1;
    double yj = lane <= k ? s[lane] : 0.0;
    double hrow[kMaxRestart];
#pragma unroll
    for (int i = 0; i < kMaxRestart; i++) hrow[i] = (lane <= k && i <= k) ? H[lane + i * ld] : 0.0;
#pragma unroll
    for (int i = kMaxRestart - 1; i >= 0; i--) {
        if (i > k) continue;                              // uniform
        if (lane == i) yj = yj / hrow[i];
        const double yi = __shfl(yj, i, 64);
        if (lane < i) yj = yj - hrow[i] * yi;
    }
    if (lane <= k) y[lane] = yj;
}

// the same for restarts above kMaxRestart: one thread, serial
__global__ void k_update_y_serial(Gate g, int m, DevState *ds, const double *H, const double *s,
                                  double *y, long long zs = 0)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    ds = zp(ds, zs, blockIdx.y);
    H = zp(H, zs, blockIdx.y);
    s = zp(s, zs, blockIdx.y);
    y = zp(y, zs, blockIdx.y);
    if (threadIdx.x != 0) return;
    const int k = (ds->done & DONE_INNER) ? ds->conv_i : ds->nit - 1;
    ds->upd_k = k;
    const int ld = m + 1;
    for (int i = 0; i <= k; i++) y[i] = s[i];
    for (int i = k; i >= 0; i--) {
        y[i] /= H[i + i * ld];
        for (int j = i - 1; j >= 0; j--) y[j] -= H[j + i * ld] * y[i];
    }
}

// acc += sum_{j<=k} V_j y_j   (ascending j, as the reference's x[i] += v*y loop)
__global__ __launch_bounds__(kBlock) void k_update_x(Gate g, const DevState *ds, const double *y,
                                                     const double *V, long long ldv, double *acc,
                                                     long long units, UnitMap um, long long zs = 0)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    ds = zp(ds, zs, blockIdx.y);
    y = zp(y, zs, blockIdx.y);
    V = zp(V, zs, blockIdx.y);
    acc = zp(acc, zs, blockIdx.y);
    const int k = ds->upd_k;
    for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units;
         u += (long long)gridDim.x * kBlock) {
        if (!unit_real(um, u)) continue;                      // padding: +0 stays +0
        double2 a = ld2(acc, u);
        // eight basis vectors' loads in flight at a time, added in ascending j
        for (int j0 = 0; j0 <= k; j0 += 8) {
            double2 vv[8];
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (j0 + q <= k) vv[q] = ld2_nt(V + (j0 + q) * ldv, u);
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (j0 + q <= k) {
                    const double yj = y[j0 + q];
                    a.x = a.x + vv[q].x * yj;
                    a.y = a.y + vv[q].y * yj;
                }
        }
        st2(acc, u, a);
    }
}

// beta = ||r|| after a restart; history; j += nit
__global__ void k_end_cycle(const double *part, int G, DevState *ds, double *hist, long long zs = 0)
{
    part = zp(part, zs, blockIdx.y);
    ds = zp(ds, zs, blockIdx.y);
    hist = zp(hist, zs, blockIdx.y);
    if (ds->done) {
        // the cycle that converged inside has applied its update: a cycle
        // enqueued behind it must not apply it again
        if (threadIdx.x == 0 && (ds->done & DONE_INNER)) ds->done |= DONE_FINAL;
        return;
    }
    double s = sum_partials(part, G);
    if (threadIdx.x == 0) {
        double beta = sqrt(s);
        double resid = beta / ds->normb;
        ds->beta = beta;
        ds->resid = resid;
        hist[ds->hist_len + ds->nit] = resid;
        ds->hist_len += ds->nit + 1;
        ds->j += ds->nit;
        if (resid < ds->tol) ds->done = DONE_RESTART;   // "<" (src/gmres.cu:686)
    }
}

}  // namespace

// ======================================================= host launchers
#ifndef GG_REDUCE_UPT
#define GG_REDUCE_UPT 4
#endif
int reduce_grid(long long units)
{
    // vectors too long for k_arnoldi_persist's registers at 1024 blocks (more
    // than 8 units per thread) reduce over kWideG blocks, two per CU, so that
    // k_arnoldi_wide can keep w on chip with the same tree
    if (units > (long long)1024 * kBlock * 8) return kWideG;
    long long g = (units + kBlock * GG_REDUCE_UPT - 1) / (kBlock * GG_REDUCE_UPT);   // >= 2*UPT elements / thread
    if (g < 1) g = 1;
    if (g > 1024) g = 1024;
    return (int)g;
}

void launch_fill_u64(unsigned long long *p, long long n, unsigned long long v, hipStream_t st, Batch bt)
{
    k_fill_u64<<<dim3(blocks_for(n, kBlock, 4096), bt.nsc), kBlock, 0, st>>>(p, n, v, bt.zs);
}
void launch_sources(int nsrc, const int *kind, const int *dptr, const double *data, int it, double h, double *u,
                    hipStream_t st)
{
    if (nsrc > 0) k_sources<<<(nsrc + kBlock - 1) / kBlock, kBlock, 0, st>>>(nsrc, kind, dptr, data, it, h, u);
}
void launch_transient_step(int n, int nsrc, const int *kind, const int *dptr, const double *data, int it,
                           double h, double *u, const int *src_ptr, const int *src_idx, const double *cdiag,
                           const double *x, double *w, hipStream_t st)
{
    launch_sources(nsrc, kind, dptr, data, it, h, u, st);
    if (n > 0)
        k_transient_rhs<<<(n + kBlock - 1) / kBlock, kBlock, 0, st>>>(n, src_ptr, src_idx, u, cdiag, x, w);
}
void launch_transient_step_csr(int n, int nsrc, const int *kind, const int *dptr, const double *data, int it,
                               double h, double *u, const int *bp, const int *bi, const double *bv,
                               const int *rp, const int *ri, const double *rv, const double *x, double *w,
                               hipStream_t st)
{
    if (nsrc > 0) k_sources<<<(nsrc + kBlock - 1) / kBlock, kBlock, 0, st>>>(nsrc, kind, dptr, data, it, h, u);
    if (n > 0)
        k_transient_rhs_csr<<<(n + kBlock - 1) / kBlock, kBlock, 0, st>>>(n, bp, bi, bv, u, rp, ri, rv, x, w);
}

void launch_taps(int ntap, const int *tap, const double *x, double *mx, double *mn, double *sm, int mode,
                 double npts, hipStream_t st)
{
    if (ntap > 0) k_taps<<<(ntap + kBlock - 1) / kBlock, kBlock, 0, st>>>(ntap, tap, x, mx, mn, sm, mode, npts);
}
void launch_gather_ports(int nport, const int *port, const double *x, double *out, hipStream_t st)
{
    if (nport > 0) k_gather_ports<<<(nport + kBlock - 1) / kBlock, kBlock, 0, st>>>(nport, port, x, out);
}

int trsv_flow_max_blocks()
{
    return std::min(resident_blocks(k_trsv_flow<false>, kBlock), resident_blocks(k_trsv_flow<true>, kBlock));
}
int ilu0_columns_max_blocks()
{
    return resident_blocks(k_ilu0_columns, kBlock);
}
void launch_ilu0_columns(int n, const int *cp, const int *ri, const double *cv0, double *cv, int *level,
                         int *done, int *err, int blocks, hipStream_t st)
{
    k_ilu0_columns<<<blocks, kBlock, 0, st>>>(n, cp, ri, cv0, cv, level, done, err);
}
int iluk_wave_max_blocks()
{
    return resident_blocks(k_iluk_wave, kBlock);
}
int iluk_wave_cap() { return kIlukCap; }
void launch_iluk_scatter(int n, const int *arp, const int *aci, const double *av, const long long *prow,
                         const int *pcol, double *val, hipStream_t st)
{
    k_iluk_scatter<<<blocks_for(n, kBlock, 8192), kBlock, 0, st>>>(n, arp, aci, av, prow, pcol, val);
}
void launch_iluk_wave(int n, const long long *prow, const int *nl, const int *pcol, double *val, double *dinv,
                      int *done, const int *rows_short, int nshort, const int *rows_long, int nlong,
                      int long_blocks, int *scratch, int *err, int blocks, hipStream_t st)
{
    k_iluk_wave<<<blocks, kBlock, 0, st>>>(n, prow, nl, pcol, val, dinv, done, rows_short, nshort, rows_long,
                                           nlong, long_blocks, scratch, err);
}
void launch_gather(const double *in, const long long *idx, double *out, long long n, hipStream_t st,
                   double *fill0, double *fill1, long long nfill)
{
    if (!fill0 || !fill1) nfill = 0;
    k_gather<<<blocks_for(std::max(n, nfill), kBlock, 8192), kBlock, 0, st>>>(
        in, idx, out, n, reinterpret_cast<unsigned long long *>(fill0), reinterpret_cast<unsigned long long *>(fill1),
        nfill);
}
void launch_copy(const double *in, double *out, long long n, hipStream_t st)
{
    k_copy<<<blocks_for(n / 2, kBlock, 8192), kBlock, 0, st>>>(in, out, n / 2);
}
void launch_dot(Gate g, const double *a, const double *b, double *part, int G, long long Ppad,
                hipStream_t st, Batch bt)
{
    k_dot<<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, a, b, part, Ppad / 2, bt.zs);
}
void launch_sub_seq(Gate g, const DevCsr &C, const double *x, const double *in, double *out,
                    hipStream_t st, double *fill0, double *fill1, int nfill)
{
    const int n = std::max(C.n, nfill);
    if (n == 0) return;
    k_sub_seq<<<blocks_for(n, kBlock, 1 << 30), kBlock, 0, st>>>(
        g, C.n, C.rp.p, C.ci.p, C.v.p, x, in, out, reinterpret_cast<unsigned long long *>(fill0),
        reinterpret_cast<unsigned long long *>(fill1), nfill);
}

void launch_sep_flow(Gate g, int ntask, const int4 *tasks, const int *rows, const SepFlow &f, int *err, hipStream_t st)
{
    if (ntask <= 0) return;
    // one block per CU at most (every waiting lane polls; all co-resident), a wave per task
    static const int cap = resident_blocks(k_sep_flow, kBlock) > 0 ? device_cus() : 0;
    GG_REQUIRE(cap > 0, GG_EHIP, "k_sep_flow cannot be resident");
    const long long need = ((long long)ntask + kBlock / 64 - 1) / (kBlock / 64);
    const int blocks = (int)std::min<long long>(cap, need);
    k_sep_flow<<<blocks, kBlock, 0, st>>>(g, ntask, tasks, rows, f, err);
}
void launch_allgather_local(const ShardPtrs &b, int P, long long off, long long cnt, hipStream_t st)
{
    if (P <= 1 || cnt == 0) return;
    k_allgather_local<<<blocks_for(P * cnt, kBlock, 8192), kBlock, 0, st>>>(b, P, off, cnt);
}
void launch_ipc_allgather(const IpcPeers &pp, int me, int P, double *buf, long long cnt,
                          unsigned long long seq, long long capd, int *err, hipStream_t st)
{
    // every rank must pick the same block count for the same cnt
    const int nb = (int)std::min<long long>(kIpcXB, std::max<long long>(1, (cnt + 2047) / 2048));
    k_ipc_allgather<<<nb, kBlock, 0, st>>>(pp, me, P, buf, cnt, seq, capd, err, nullptr, nullptr, nullptr, nullptr,
                                           0);
}
void launch_ipc_gather_allgather(const IpcPeers &pp, int me, int P, const double *x, const long long *gidx,
                                 double *buf, long long cnt, unsigned long long seq, long long capd, int *err,
                                 double *f0, double *f1, long long nf, hipStream_t st)
{
    // the block count depends on cnt only, as launch_ipc_allgather's (every rank the same)
    const int nb = (int)std::min<long long>(kIpcXB, std::max<long long>(1, (cnt + 2047) / 2048));
    if (!f0 || !f1) nf = 0;
    k_ipc_allgather<<<nb, kBlock, 0, st>>>(pp, me, P, buf, cnt, seq, capd, err, x, gidx,
                                           reinterpret_cast<unsigned long long *>(f0),
                                           reinterpret_cast<unsigned long long *>(f1), nf);
}
bool launch_dd_spmv_x(Gate g, const DdSpmvCall &c, hipStream_t st)
{
    const DevCsr &AI = *c.AI, &AS = *c.AS;
    if (AI.panel || AS.panel || c.P < 2 || c.P > kMaxShards) return false;
    DdSpmvX a{};
    a.pp = c.pp;
    a.me = c.me;
    a.P = c.P;
    a.loop = c.loop ? 1 : 0;
    a.halo = c.halo;
    a.cnt = c.cnt;
    a.capd = c.capd;
    a.seq = c.seq;
    a.err = c.err;
    a.gidx = c.gidx;
    a.arrived = c.arrived;
    // the exchange's block count depends on cnt only (every rank the same, as
    // launch_ipc_gather_allgather's); loopback: k_gather_allgather_local's span
    a.nbx = c.loop ? (int)std::min<long long>(kIpcXB, std::max<long long>(1, ((long long)c.P * c.cnt + 2047) / 2048))
                   : (int)std::min<long long>(kIpcXB, std::max<long long>(1, (c.cnt + 2047) / 2048));
    a.target = c.epoch * (unsigned long long)a.nbx;
    auto rows = [](const DevCsr &A, int &sell, int &n, int &nb, const int *&ptr, const int *&rp, const int *&ci,
                   const double *&v) {
        sell = A.sell ? 1 : 0;
        n = A.n;
        if (A.sell) {
            nb = A.nslice;
            ptr = A.sptr.p;
            rp = nullptr;
            ci = A.sci.p;
            v = A.sv.p;
            return (A.nslice + kBlock / 64 - 1) / (kBlock / 64);
        }
        nb = A.nblk;
        ptr = A.blk.p;
        rp = A.rp.p;
        ci = A.ci.p;
        v = A.v.p;
        return A.nblk;
    };
    a.nbi = AI.nblk == 0 ? 0 : rows(AI, a.i_sell, a.i_n, a.i_nb, a.i_ptr, a.i_rp, a.i_ci, a.i_v);
    a.nbs = AS.nblk == 0 ? 0 : rows(AS, a.s_sell, a.s_n, a.s_nb, a.s_ptr, a.s_rp, a.s_ci, a.s_v);
    a.x = c.x;
    a.b = c.b;
    a.y = c.y;
    a.S0 = c.S0;
    const int grid = a.nbx + a.nbi + a.nbs;
    if (c.resid) k_dd_spmv_x<true><<<grid, kBlock, 0, st>>>(g, a);
    else k_dd_spmv_x<false><<<grid, kBlock, 0, st>>>(g, a);
    return true;
}
void launch_gather_allgather_local(const ShardPtrs &b, const IdxPtrs &gi, int P, long long off, long long cnt,
                                   const FillPtrs &fl, long long nf, hipStream_t st)
{
    if (P * cnt == 0 && nf == 0) return;
    k_gather_allgather_local<<<blocks_for(std::max(P * cnt, nf), kBlock, 8192), kBlock, 0, st>>>(b, gi, P, off, cnt,
                                                                                             fl, nf);
}
void launch_scatter_idx(const double *in, const long long *src, const long long *dst, double *out,
                        long long n, hipStream_t st)
{
    if (n == 0) return;
    k_scatter_idx<<<blocks_for(n, kBlock, 8192), kBlock, 0, st>>>(in, src, dst, out, n);
}

void launch_fingerprint(const void *p, long long nw, unsigned long long *out, hipStream_t st)
{
    if (nw <= 0) return;
    k_fingerprint<<<blocks_for(nw, kBlock, 2048), kBlock, 0, st>>>(static_cast<const unsigned *>(p), nw, out);
}
void launch_f64_to_f32(Gate g, const double *in, float *out, int n, hipStream_t st)
{
    k_f64_to_f32<<<blocks_for(n, kBlock, 1 << 30), kBlock, 0, st>>>(g, in, out, n);
}
void launch_f32_to_f64(Gate g, const float *in, double *out, int n, hipStream_t st)
{
    k_f32_to_f64<<<blocks_for(n, kBlock, 1 << 30), kBlock, 0, st>>>(g, in, out, n);
}
void launch_mul(Gate g, const double *in, const double *s, double *out, int n, hipStream_t st)
{
    k_mul<<<blocks_for(n, kBlock, 1 << 30), kBlock, 0, st>>>(g, in, s, out, n);
}
void launch_div(Gate g, const double *in, const double *s, double *out, int n, hipStream_t st)
{
    k_div<<<blocks_for(n, kBlock, 1 << 30), kBlock, 0, st>>>(g, in, s, out, n);
}

void launch_spmv(Gate g, const DevCsr &A, const double *x, const double *b, double *y, bool resid,
                 hipStream_t st, const double *ydiv, const double *ymul)
{
    if (A.nblk == 0) return;
    if (ymul) {
        // y = (A x) o ymul (AINV's first product): the sliced or the CSR-stream kernel
        if (A.sell)
            k_spmv_sell_mul<<<(A.nslice + kBlock / 64 - 1) / (kBlock / 64), kBlock, 0, st>>>(
                g, A.n, A.nslice, A.sptr.p, A.sci.p, A.sv.p, x, y, ymul);
        else
            k_spmv_stream_mul<<<A.nblk, kBlock, 0, st>>>(g, A.blk.p, A.rp.p, A.ci.p, A.v.p, x, y, ymul);
        return;
    }
    if (A.panel && A.rtile && !resid && !ydiv && x != y) {
        // row tiles: one launch, each block its rows' segments panel by panel
        k_spmv_rtile<<<A.rtile, kBlock, 0, st>>>(g, A.rt_sub.p, A.pblk.p, A.seg_row.p, A.seg_ptr.p, A.pci.p, A.pv.p, x,
                                                  y, A.zero_rows.p, A.nzero);
        return;
    }
    if (A.panel && !resid && !ydiv && x != y) {
        // column panels: one launch per panel over its segment blocks
        for (int p = 0; p < A.npanel; p++) {
            const int nb = A.pan_blk_h[p + 1] - A.pan_blk_h[p];
            if (nb > 0)
                k_spmv_panel<<<nb, kBlock, 0, st>>>(g, A.pblk.p + A.pan_blk_h[p], A.seg_row.p, A.seg_ptr.p, A.pci.p,
                                                     A.pv.p, x, y, A.zero_rows.p, p == 0 ? A.nzero : 0);
        }
        return;
    }
#define GG_SPMV(R, D)                                                                                  \
    do {                                                                                               \
        if (A.sell)                                                                                    \
            k_spmv_sell<R, D><<<(A.nslice + kBlock / 64 - 1) / (kBlock / 64), kBlock, 0, st>>>(        \
                g, A.n, A.nslice, A.sptr.p, A.sci.p, A.sv.p, x, b, y, ydiv, nullptr);                  \
        else                                                                                           \
            k_spmv_stream<R, D><<<A.nblk, kBlock, 0, st>>>(g, A.blk.p, A.rp.p, A.ci.p, A.v.p, x, b, y, \
                                                          ydiv);                                       \
    } while (0)
    if (ydiv) {
        if (resid) GG_SPMV(true, true);
        else GG_SPMV(false, true);
    } else {
        if (resid) GG_SPMV(true, false);
        else GG_SPMV(false, false);
    }
#undef GG_SPMV
}

bool launch_spmv_xdiv(Gate g, const DevCsr &A, const double *x, const double *xdiv, double *y, hipStream_t st,
                      const double *ydiv, double *fill, int nfill)
{
    if (!A.sell || !ydiv) return false;
    // the caller relies on the fill having happened (DevTri::prefilled): when
    // it cannot ride on the SpMV's lanes it gets a launch of its own
    if (fill && (A.nblk == 0 || nfill > A.nslice * 64)) {
        k_fill_gated<<<blocks_for(nfill, kBlock, 8192), kBlock, 0, st>>>(
            g, reinterpret_cast<unsigned long long *>(fill), nfill, kSentinel);
        fill = nullptr;
    }
    if (A.nblk == 0) return true;
    if (!fill) nfill = 0;
    k_spmv_sell<false, true, true><<<(A.nslice + kBlock / 64 - 1) / (kBlock / 64), kBlock, 0, st>>>(
        g, A.n, A.nslice, A.sptr.p, A.sci.p, A.sv.p, x, nullptr, y, ydiv, xdiv,
        reinterpret_cast<unsigned long long *>(fill), fill ? nfill : 0);
    return true;
}

void launch_trsv(Gate g, DevTri &T, const double *b, double *x, int *err, hipStream_t st)
{
    if (!T.tail) {
        launch_trsv_one(g, T, b, x, err, st);
        return;
    }
    // bordered grid: tail, coupling, grid (forward); grid, tail (backward)
    const int e = T.eff_div();
    const bool fm = e == WD_UFMA || e == WD_SFMA;
    // the tail rows divide as the grid's do (GG_DIV_FMA: the fused-order copy)
    DevTri &tl = fm ? *T.tail_fma : *T.tail;
    tl.fast = 0;
    tl.mul = e == WD_MUL;
    if (tl.lev_ptr_d.p) {
        // a small tail: one workgroup for the tail and the coupling
        auto tail_small = [&](bool coup) {
            k_tail_small<<<1, 1024, 0, st>>>(g, (int)tl.lev_ptr.size() - 1, tl.lev_ptr_d.p, tl.lev_rows.p,
                                             tl.off.rp.p, tl.off.ci.p, tl.off.v.p, tl.d.p,
                                             (tl.mul || tl.fmrow) ? tl.rw.p : nullptr, tl.fmrow ? 1 : 0, b, x,
                                             coup ? T.ncoup : 0, T.cslot.p, T.crp.p, T.cci.p, T.cv.p,
                                             const_cast<double *>(b), fm ? 1 : 0);
        };
        if (T.lower) {
            tail_small(true);
            launch_trsv_one(g, T, b + T.bofs, x + T.bofs, err, st);
        } else {
            launch_trsv_one(g, T, b + T.bofs, x + T.bofs, err, st);
            tail_small(false);
        }
        return;
    }
    if (T.lower) {
        launch_trsv_one(g, tl, b, x, err, st);
        if (T.ncoup)
            k_border_sub<<<(T.ncoup + kBlock - 1) / kBlock, kBlock, 0, st>>>(
                g, T.ncoup, T.cslot.p, T.crp.p, T.cci.p, T.cv.p, x, const_cast<double *>(b), fm ? 1 : 0);
        launch_trsv_one(g, T, b + T.bofs, x + T.bofs, err, st);
    } else {
        launch_trsv_one(g, T, b + T.bofs, x + T.bofs, err, st);
        launch_trsv_one(g, tl, b, x, err, st);
    }
}

// the level-scheduled triangle T (DevTri::LEVEL): one dataflow launch, or a launch per level
void launch_trsv_levels(Gate g, DevTri &T, const double *b, double *x, int *err, hipStream_t st)
{
    const int nlev = (int)T.lev_ptr.size() - 1;
    static const int flow_blocks = trsv_flow_max_blocks();
    const char *lv = getenv("GG_TRSV_LEVELS");         // 1: one launch per level
    const bool per_level = lv && atoi(lv) != 0;
    const int nrows = T.lev_ptr[nlev];
    if (!per_level && b != x && flow_blocks > 0 && nlev > 1 && nrows > 0) {
        // few resident waves: every waiting lane polls, so the grid is
        // capped at GG_FLOW_BPC blocks per CU (default 1)
        static const int cus = device_cus();
        // one block per CU where the levels are narrow (every waiting lane
        // polls; more pollers slow the hand-offs), up to occupancy where a
        // level holds more tasks than 4 waves per CU can take (C3: 3,100
        // tasks per level, 0.66 ms per solve at 8 blocks per CU vs 2.1 ms at 1)
        const char *bpc_s = getenv("GG_FLOW_BPC");
        const long long per_level = (T.ntask + nlev - 1) / std::max(nlev, 1);
        const long long wave_slots = 4LL * std::max(cus, 1);          // 4 waves per block, 1 block per CU
        // (the randomly permuted PG split, 1,100 tasks per level: 2 blocks per
        // CU 84 / 102 us for L / U against 95 / 127 at 4 and 102 / 131 at 8,
        // profiles/r04/r04s_pgr_bpc*.json -- so the extra factor 2 only beyond
        // two waves per slot)
        const long long wpl = (per_level + wave_slots - 1) / wave_slots;
        const int bpc = bpc_s ? std::max(1, atoi(bpc_s))
                              : per_level <= wave_slots ? 1
                              : (int)std::min<long long>(8, per_level > 2 * wave_slots ? 2 * wpl : wpl);
        const long long need = ((long long)T.ntask + kBlock / 64 - 1) / (kBlock / 64);   // a wave per task
        const int blocks = (int)std::min<long long>(std::min<long long>(flow_blocks, (long long)bpc * std::max(cus, 1)), need);
        if (!T.prefilled)
            k_fill_gated<<<blocks_for(nrows, kBlock, 8192), kBlock, 0, st>>>(
                g, reinterpret_cast<unsigned long long *>(x), nrows, kSentinel);
        if (T.ell)
            k_trsv_flow<true><<<blocks, kBlock, 0, st>>>(g, T.ntask, T.tasks.p, T.lev_rows.p, T.off.rp.p,
                                                         T.off.ci.p, T.off.v.p, T.d.p, b, x, err,
                                                         (T.mul || T.fmrow) ? T.rw.p : nullptr, T.fmrow ? 1 : 0,
                                                         T.eci.p, T.ev.p);
        else
            k_trsv_flow<false><<<blocks, kBlock, 0, st>>>(g, T.ntask, T.tasks.p, T.lev_rows.p, T.off.rp.p,
                                                          T.off.ci.p, T.off.v.p, T.d.p, b, x, err,
                                                          (T.mul || T.fmrow) ? T.rw.p : nullptr, T.fmrow ? 1 : 0,
                                                          nullptr, nullptr);
        return;
    }
    for (int l = 0; l < nlev; l++) {
        const int cnt = T.lev_ptr[l + 1] - T.lev_ptr[l];
        if (cnt == 0) continue;
        k_trsv_level<<<(cnt + kBlock - 1) / kBlock, kBlock, 0, st>>>(
            g, cnt, T.lev_rows.p + T.lev_ptr[l], T.off.rp.p, T.off.ci.p, T.off.v.p, T.d.p, b, x,
            (T.mul || T.fmrow) ? T.rw.p : nullptr, T.fmrow ? 1 : 0);
    }
}

void launch_set_normb(const double *part, int G, DevState *ds, hipStream_t st, Batch bt)
{
    k_set_normb<<<dim3(1, bt.nsc), kBlock, 0, st>>>(part, G, ds, bt.zs);
}
void launch_init_beta(const double *part, int G, DevState *ds, double *hist, hipStream_t st, Batch bt)
{
    k_init_beta<<<dim3(1, bt.nsc), kBlock, 0, st>>>(part, G, ds, hist, bt.zs);
}
void launch_init_cycle(DevState *ds, const double *r, double *v0, double *s, int G, long long Ppad,
                       hipStream_t st, Batch bt)
{
    k_init_cycle<<<dim3(G, bt.nsc), kBlock, 0, st>>>(ds, r, v0, s, Ppad / 2, bt.zs);
}
void launch_mgs_step(Gate g, int i, int k, int m, double *w, const double *vk, const double *vnext,
                     const double *part_in, double *part_out, double *H, int G, long long Ppad,
                     hipStream_t st, Batch bt)
{
    launch_mgs_step_r(g, i, k, m, w, vk, vnext, part_in, G, part_out, H, G, Ppad, Ppad, st, bt);
}
void launch_mgs_step_r(Gate g, int i, int k, int m, double *w, const double *vk, const double *vnext,
                       const double *part_in, int nparts_in, double *part_out, double *H, int G,
                       long long Ppad, long long Pdot, hipStream_t st, Batch bt)
{
    if (vnext == w)
        k_mgs_step<true><<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, i, k, m, w, vk, nullptr, part_in, part_out, H,
                                                             nparts_in, Ppad / 2, Pdot / 2, bt.zs);
    else
        k_mgs_step<false><<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, i, k, m, w, vk, vnext, part_in, part_out, H,
                                                              nparts_in, Ppad / 2, Pdot / 2, bt.zs);
}
void launch_multidot(Gate g, const double *w, const double *V, long long ldv, int nk, double *part, int G,
                     long long Pdot, hipStream_t st)
{
    dim3 grid(G, (nk + kCgsKC - 1) / kCgsKC);
    k_multidot<<<grid, kBlock, 0, st>>>(g, w, V, ldv, nk, part, G, Pdot / 2);
}
void launch_cgs_reduce(Gate g, const double *part, int P, int G, long long cnt, int nk, double *h, double *H,
                       int i, int m, bool add, hipStream_t st)
{
    k_cgs_reduce<<<nk, kBlock, 0, st>>>(g, part, P, G, cnt, h, H, i, m, add ? 1 : 0);
}
void launch_cgs_update(Gate g, double *w, const double *V, long long ldv, const double *h, int nk, int G,
                       long long Ppad, long long Pdot, double *part_norm, hipStream_t st)
{
    if (part_norm)
        k_cgs_update<true><<<G, kBlock, 0, st>>>(g, w, V, ldv, h, nk, Ppad / 2, Pdot / 2, part_norm);
    else
        k_cgs_update<false><<<G, kBlock, 0, st>>>(g, w, V, ldv, h, nk, Ppad / 2, Pdot / 2, nullptr);
}
bool launch_cgs_update_dot(Gate g, double *w, const double *V, long long ldv, const double *h, int nk, int G,
                           long long Ppad, long long Pdot, double *part, hipStream_t st)
{
    if (nk > kCgsFuseMax) return false;
    k_cgs_update_dot<<<G, kBlock, 0, st>>>(g, w, V, ldv, h, nk, Ppad / 2, Pdot / 2, part, G);
    return true;
}
void launch_arnoldi_finalize(Gate g, int i, int m, DevState *ds, const double *part, int G,
                             const double *w, double *vnext, double *H, double *cs, double *sn,
                             double *s, double *hist, long long Ppad, hipStream_t st, Batch bt)
{
    launch_arnoldi_finalize_r(g, i, m, ds, part, G, G, w, vnext, H, cs, sn, s, hist, Ppad, st, bt);
}
void launch_arnoldi_finalize_r(Gate g, int i, int m, DevState *ds, const double *part, int nparts_in,
                               int G, const double *w, double *vnext, double *H, double *cs,
                               double *sn, double *s, double *hist, long long Ppad, hipStream_t st, Batch bt)
{
    k_arnoldi_finalize<<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, i, m, ds, part, nparts_in, w, vnext, H, cs, sn, s,
                                                           hist, Ppad / 2, bt.zs);
}
size_t xch_area_bytes(int P, long long capd)
{
    return sizeof(double) * ((size_t)kMaxShards * kIpcXB + 2ull * P * capd + (size_t)kMaxShards * kIpcXF);
}
void launch_multidot_x(Gate g, const double *w, const double *V, long long ldv, int nk, double *part, int G,
                       long long Pdot, const Xch &x, unsigned long long seq, hipStream_t st)
{
    // (the caller checks nk <= kCgsXMax, G <= kIpcXF, nk * G <= x.capd)
    k_multidot_x<<<dim3(G, (nk + kCgsKC - 1) / kCgsKC), kBlock, 0, st>>>(g, w, V, ldv, nk, part, G, Pdot / 2, x, seq);
}
void launch_cgs_update_x(Gate g, double *w, const double *V, long long ldv, int nk, int G, long long Ppad,
                         long long Pdot, const double *part_in, unsigned long long sin, double *H, int i, int m,
                         bool add, double *part_out, double *norm_out, const Xch &x, unsigned long long sout,
                         hipStream_t st)
{
    if (part_out)
        k_cgs_update_x<true><<<G, kBlock, 0, st>>>(g, w, V, ldv, nk, Ppad / 2, Pdot / 2, G, part_in, sin, H, i, m,
                                                    add ? 1 : 0, part_out, x, sout, add ? 0 : kCgsKC);
    else
        k_cgs_update_x<false><<<G, kBlock, 0, st>>>(g, w, V, ldv, nk, Ppad / 2, Pdot / 2, G, part_in, sin, H, i,
                                                     m, add ? 1 : 0, norm_out, x, sout, add ? 0 : kCgsKC);
}
void launch_dot_x(Gate g, const double *a, const double *b, double *part, int G, long long Pdot, const Xch &x,
                  unsigned long long seq, hipStream_t st)
{
    k_dot_x<<<G, kBlock, 0, st>>>(g, a, b, part, Pdot / 2, x, seq);
}
void launch_mgs_step_x(Gate g, int i, int k, int m, double *w, const double *vk, const double *vnext,
                       const double *part_in, unsigned long long sin, double *part_out, double *H, int G,
                       long long Ppad, long long Pdot, const Xch &x, unsigned long long sout, hipStream_t st)
{
    if (!vnext)
        k_mgs_step_x<true><<<G, kBlock, 0, st>>>(g, i, k, m, w, vk, nullptr, part_in, sin, part_out, H, G, Ppad / 2,
                                                  Pdot / 2, x, sout);
    else
        k_mgs_step_x<false><<<G, kBlock, 0, st>>>(g, i, k, m, w, vk, vnext, part_in, sin, part_out, H, G, Ppad / 2,
                                                   Pdot / 2, x, sout);
}
void launch_arnoldi_finalize_x(Gate g, int i, int m, DevState *ds, const double *part_in, unsigned long long sin,
                               int G, const double *w, double *vnext, double *H, double *cs, double *sn,
                               double *s, double *hist, long long Ppad, const Xch &x, hipStream_t st)
{
    k_arnoldi_finalize_x<<<G, kBlock, 0, st>>>(g, i, m, ds, part_in, sin, G, w, vnext, H, cs, sn, s, hist,
                                                Ppad / 2, x);
}

void launch_update(Gate g, int m, DevState *ds, const double *H, const double *s, double *ysmall,
                   const double *V, long long ldv, double *acc, int G, long long Ppad, hipStream_t st,
                   const UnitMap &um, Batch bt)
{
    if (m <= kMaxRestart) k_update_y<<<dim3(1, bt.nsc), 64, 0, st>>>(g, m, ds, H, s, ysmall, bt.zs);
    else k_update_y_serial<<<dim3(1, bt.nsc), 64, 0, st>>>(g, m, ds, H, s, ysmall, bt.zs);
    k_update_x<<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, ds, ysmall, V, ldv, acc, Ppad / 2, um, bt.zs);
}
void launch_end_cycle(const double *part, int G, DevState *ds, double *hist, hipStream_t st, Batch bt)
{
    k_end_cycle<<<dim3(1, bt.nsc), kBlock, 0, st>>>(part, G, ds, hist, bt.zs);
}

void launch_gather_b(const double *in, long long zin, const long long *idx, double *out, long long zout,
                     long long n, int nsc, hipStream_t st)
{
    k_gather_b<<<dim3(blocks_for(n, kBlock, 4096), nsc), kBlock, 0, st>>>(in, zin, idx, out, zout, n);
}
void launch_init_state_b(DevState *ds, long long zs, int nsc, double tol, int max_iter, int m, hipStream_t st)
{
    k_init_state_b<<<(nsc + 63) / 64, 64, 0, st>>>(ds, zs, nsc, tol, max_iter, m);
}
template <class State>
void launch_pack_states_b(const State *st0, long long zs, int nsc, State *out, const int *err, hipStream_t st)
{
    k_pack_states_b<State><<<(nsc + 64) / 64, 64, 0, st>>>(st0, zs, nsc, out, err);
}
template void launch_pack_states_b<DevState>(const DevState *, long long, int, DevState *, const int *, hipStream_t);
template void launch_pack_states_b<CgState>(const CgState *, long long, int, CgState *, const int *, hipStream_t);
template void launch_pack_states_b<BiState>(const BiState *, long long, int, BiState *, const int *, hipStream_t);
void launch_transient_step_b(int n, int nsc, int maxsrc, const int *soff, const int *kind, const int *dptr,
                             const double *data, int it, double h, double *u, const int *sptr, const int *sidx,
                             const double *cdiag, const double *x, double *w, long long ldx, hipStream_t st)
{
    if (maxsrc > 0) k_sources_b<<<dim3((maxsrc + kBlock - 1) / kBlock, nsc), kBlock, 0, st>>>(soff, kind, dptr, data, it, h, u);
    if (n > 0) k_transient_rhs_b<<<dim3((n + kBlock - 1) / kBlock, nsc), kBlock, 0, st>>>(n, sptr, sidx, u, cdiag, x, w, ldx);
}
void launch_gather_ports_b(int nport, const int *port, const double *x, long long ldx, double *out, long long ldo,
                           int nsc, hipStream_t st)
{
    if (nport > 0)
        k_gather_ports_b<<<dim3((nport + kBlock - 1) / kBlock, nsc), kBlock, 0, st>>>(nport, port, x, ldx, out, ldo);
}
void launch_spmv_b(Gate g, const DevCsr &A, const double *x, const double *b, double *y, bool resid, int nsc,
                   long long zs, hipStream_t st)
{
    if (A.nblk == 0) return;
    if (!A.sell) {
        // CSR-stream (no sliced copy): one launch per scenario, the same kernel
        for (int q = 0; q < nsc; q++) {
            const long long o = (long long)q * zs;
            auto at = [o](auto *p) { return p ? reinterpret_cast<decltype(p)>(reinterpret_cast<char *>(const_cast<void *>(static_cast<const void *>(p))) + o) : p; };
            Gate gq = g;
            gq.done = at(g.done);
            gq.nit = at(g.nit);
            launch_spmv(gq, A, at(x), resid ? at(b) : nullptr, at(y), resid, st);
        }
        return;
    }
    const int blocks = (A.nslice + kBlock / 64 - 1) / (kBlock / 64);
    // up to 8 scenarios per launch (A's entries read once for all of them)
    for (int q0 = 0; q0 < nsc; q0 += kBatchSpmv) {
        const int c = std::min(kBatchSpmv, nsc - q0);
        const long long o = (long long)q0 * zs;
        auto at = [o](auto *p) { return p ? reinterpret_cast<decltype(p)>(reinterpret_cast<char *>(const_cast<void *>(static_cast<const void *>(p))) + o) : p; };
        Gate gq = g;
        gq.done = at(g.done);
        gq.nit = at(g.nit);
        if (resid)
            k_spmv_sell_b<true, kBatchSpmv><<<blocks, kBlock, 0, st>>>(gq, zs, c, A.n, A.nslice, A.sptr.p, A.sci.p,
                                                                       A.sv.p, at(x), at(b), at(y));
        else
            k_spmv_sell_b<false, kBatchSpmv><<<blocks, kBlock, 0, st>>>(gq, zs, c, A.n, A.nslice, A.sptr.p, A.sci.p,
                                                                        A.sv.p, at(x), nullptr, at(y));
    }
}

}  // namespace gg
