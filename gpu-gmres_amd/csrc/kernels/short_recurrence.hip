// short_recurrence.hip -- the CG and BiCGStab kernels.
#include "device.h"
#include "host.h"

namespace gg {

namespace {

// ================================================================ CG kernels
// Left-preconditioned conjugate gradients (cg.hip; DESIGN.md "CG").  Besides
// the SpMV and the preconditioner an iteration is four launches, each in
// k_mgs_step's form: the previous launch's G partials summed redundantly in
// every block (sum_partials: the same bits everywhere), the scalar formed,
// the vectors streamed kUnroll 16-B units per stream in flight, partials left
// for the next launch.  Every dot keeps k_dot's order (thread t of block b:
// units b*256 + t + j*G*256 ascending, block_sum's tree).  No atomics; the
// control block is written by thread 0 of block 0 alone, and a word a launch
// writes is read by no other block of that launch except the done bits -- a
// block that sees them early returns where it would have returned anyway
// (every block forms the same scalars).  rz alternates between two words: the
// launch that forms iteration it's beta from rz[it & 1] stores the next one.
// (k_normb, k_cg_pq and k_cg_rz touch no control block: BiCGStab launches them too.)
// zs: the many-RHS batch (cg_batch.hip, bicgstab_batch.hip), as k_dot -- grid
// (G, nsc), blockIdx.y = scenario, every per-scenario pointer (vectors,
// partials, control block,
// history, the gate's words) blockIdx.y * zs bytes on; the control block is
// then written by thread 0 of block (0, scenario).  zs = 0: the single solve.
//
// The sharded solve (dd.hip "Sharded CG") runs the same kernels on a shard's
// vector: grid G, the updates over the shard's H0 slots, a dot over its dot
// range alone (k_cg_pq, k_cg_rz: units = the dot range), its G partials written
// into the shard's slot of an all-gathered array.  A consumer then sums P * G
// partials shard-major: k_cg_xr takes the p.q slots, G doubles each and so
// contiguous, as G = P * G; k_cg_p<START, true> takes the paired dot's slots,
// 2 G doubles each -- r.z's G, then z.z's -- through sum_partials_sh.
//
// Sum of the P * G partials in P slots of `slot` doubles (shard q's G at part +
// q * slot): sum_partials' order over the values taken shard-major, identical
// in every block.  slot = G: sum_partials(part, P * G).
__device__ __forceinline__ double sum_partials_sh(const double *part, int P, int G, long long slot)
{
    double v = 0.0;
    const int n = P * G;
    for (int k = threadIdx.x; k < n; k += kBlock) {
        const int q = k / G;
        v += part[q * slot + (k - q * G)];
    }
    return block_sum(v);
}

__global__ void k_normb(const double *part, int G, double *normb, long long zs = 0)
{
    part = zp(part, zs, blockIdx.y);
    normb = zp(normb, zs, blockIdx.y);
    const double s = sum_partials(part, G);
    if (threadIdx.x == 0) {
        const double nb = sqrt(s);
        *normb = (nb == 0.0) ? 1.0 : nb;
    }
}

// block partials of p . q
__global__ __launch_bounds__(kBlock) void k_cg_pq(Gate g, const double *__restrict__ p,
                                                  const double *__restrict__ q, double *part, long long units,
                                                  long long zs = 0)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    p = zp(p, zs, blockIdx.y);
    q = zp(q, zs, blockIdx.y);
    part = zp(part, zs, blockIdx.y);
    double acc = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x; u0 < units; u0 += kUnroll * stride) {
        double2 a[kUnroll], b[kUnroll];
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) { a[j] = ld2(p, u); b[j] = ld2(q, u); }
        }
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            if (u0 + j * stride < units) {
                acc += a[j].x * b[j].x;
                acc += a[j].y * b[j].y;
            }
        }
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// pq from the partials; alpha = rz / pq (breakdown unless pq > 0, NaN included);
// x = alpha p + x;  r = (-alpha) q + r
__global__ __launch_bounds__(kBlock) void k_cg_xr(Gate g, int it, CgState *cs, const double *part, int G,
                                                  double *__restrict__ x, const double *__restrict__ p,
                                                  double *__restrict__ r, const double *__restrict__ q,
                                                  long long units, long long zs = 0)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    cs = zp(cs, zs, blockIdx.y);
    part = zp(part, zs, blockIdx.y);
    x = zp(x, zs, blockIdx.y);
    p = zp(p, zs, blockIdx.y);
    r = zp(r, zs, blockIdx.y);
    q = zp(q, zs, blockIdx.y);
    const long long stride = (long long)gridDim.x * kBlock;
    long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x;
    double2 xv[kUnroll], pv[kUnroll], rv[kUnroll], qv[kUnroll];
    auto load = [&]() {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                xv[j] = ld2(x, u);
                pv[j] = ld2(p, u);
                rv[j] = ld2(r, u);
                qv[j] = ld2(q, u);
            }
        }
    };
    load();                 // the first chunk is in flight while pq is summed
    const double pq = sum_partials(part, G);
    const double rz = cs->rz[it & 1];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (!(pq > 0.0)) {
        if (first) cs->done = SR_BREAKDOWN;
        return;
    }
    const double alpha = rz / pq;
    if (first) cs->alpha = alpha;
    const double na = -alpha;
    while (u0 < units) {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                xv[j].x = alpha * pv[j].x + xv[j].x;
                xv[j].y = alpha * pv[j].y + xv[j].y;
                rv[j].x = na * qv[j].x + rv[j].x;
                rv[j].y = na * qv[j].y + rv[j].y;
                st2(x, u, xv[j]);
                st2(r, u, rv[j]);
            }
        }
        u0 += kUnroll * stride;
        load();
    }
}

// block partials of r . z (part[b]) and z . z (part[G + b]) in one pass
__global__ __launch_bounds__(kBlock) void k_cg_rz(Gate g, const double *__restrict__ r,
                                                  const double *__restrict__ z, double *part, long long units,
                                                  long long zs = 0)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    r = zp(r, zs, blockIdx.y);
    z = zp(z, zs, blockIdx.y);
    part = zp(part, zs, blockIdx.y);
    double acc[2] = {0.0, 0.0};
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x; u0 < units; u0 += kUnroll * stride) {
        double2 a[kUnroll], b[kUnroll];
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) { a[j] = ld2(r, u); b[j] = ld2(z, u); }
        }
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            if (u0 + j * stride < units) {
                acc[0] += a[j].x * b[j].x;
                acc[0] += a[j].y * b[j].y;
                acc[1] += b[j].x * b[j].x;
                acc[1] += b[j].y * b[j].y;
            }
        }
    }
    block_sum_store<2>(acc, 2, part + blockIdx.x, gridDim.x);
}

// rzn, zz from the partials; res = sqrt(zz) / normb into the history; converged
// (START: res <= tol, else res < tol), breakdown (not converged and not rzn > 0,
// NaN included); otherwise p = beta p + z with beta = rzn / rz (START: p = z).
// it: the iteration's 0-based index (START: the initial residual, nothing counted)
// SH: the sharded solve -- part holds P slots of 2 G doubles (above)
template <bool START, bool SH = false>
__global__ __launch_bounds__(kBlock) void k_cg_p(Gate g, int it, CgState *cs, const double *part, int G,
                                                 double *__restrict__ p, const double *__restrict__ z,
                                                 double *hist, long long units, long long zs = 0, int P = 1)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    cs = zp(cs, zs, blockIdx.y);
    part = zp(part, zs, blockIdx.y);
    p = zp(p, zs, blockIdx.y);
    z = zp(z, zs, blockIdx.y);
    hist = zp(hist, zs, blockIdx.y);
    const long long stride = (long long)gridDim.x * kBlock;
    long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x;
    double2 pv[kUnroll], zv[kUnroll];
    auto load = [&]() {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                zv[j] = ld2(z, u);
                if (!START) pv[j] = ld2(p, u);
            }
        }
    };
    load();
    const double rzn = SH ? sum_partials_sh(part, P, G, 2LL * G) : sum_partials(part, G);
    const double zz = SH ? sum_partials_sh(part + G, P, G, 2LL * G) : sum_partials(part + G, G);
    const double res = sqrt(zz) / cs->normb;
    const bool conv = START ? res <= cs->tol : res < cs->tol;
    const bool brk = !conv && !(rzn > 0.0);
    const int done_it = START ? 0 : it + 1;            // iterations performed
    const double rz = START ? 0.0 : cs->rz[it & 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cs->resid = res;
        hist[done_it] = res;
        cs->it = done_it;
        cs->rz[done_it & 1] = rzn;
        if (conv) cs->done = START ? SR_INIT : SR_CONV;
        else if (brk) cs->done = SR_BREAKDOWN;
    }
    if (conv || brk) return;
    const double beta = START ? 0.0 : rzn / rz;
    while (u0 < units) {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                if (!START) {
                    zv[j].x = beta * pv[j].x + zv[j].x;
                    zv[j].y = beta * pv[j].y + zv[j].y;
                }
                st2(p, u, zv[j]);
            }
        }
        u0 += kUnroll * stride;
        load();
    }
}

// ========================================================== BiCGStab kernels
// Left-preconditioned BiCGStab (bicgstab.hip; DESIGN.md "BiCGStab").  Besides
// the two SpMVs and the two preconditioner applications an iteration is five
// launches in the CG kernels' form: k_cg_pq (rt . v), k_bi_s, k_cg_rz (t . s
// and t . t), k_bi_xr, k_bi_p.  The same rules: partials summed redundantly in
// every block, the scalar formed in every block, kUnroll 16-B units per stream
// in flight, k_dot's order in every dot, no atomics, the control block written
// by thread 0 of block 0 alone.  alpha and omega are stored by one launch and
// read by later ones only; rho alternates between two words like CG's rz.
// zs: the many-RHS batch (bicgstab_batch.hip), as the CG kernels above.
//
// The sharded solve (dd.hip "Sharded BiCGStab") runs them as it runs CG's: grid
// G per shard, the updates over the shard's H0 slots, a dot over its dot range
// alone, its partials in the shard's slot of an all-gathered array.  k_bi_s
// takes rt.v's slots, G doubles each and so contiguous, as G = P * G;
// k_bi_xr<true> and k_bi_p<START, true> take the paired dots' slots, 2 G
// doubles each, through sum_partials_sh.
__device__ __forceinline__ bool bi_bad(double v) { return !isfinite(v) || v == 0.0; }

// rtv from the partials (breakdown when zero or not finite: nothing moves);
// alpha = rho / rtv;  s = (-alpha) v + r in place of r
__global__ __launch_bounds__(kBlock) void k_bi_s(Gate g, int it, BiState *bs, const double *part, int G,
                                                 double *__restrict__ r, const double *__restrict__ v,
                                                 long long units, long long zs = 0)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    bs = zp(bs, zs, blockIdx.y);
    part = zp(part, zs, blockIdx.y);
    r = zp(r, zs, blockIdx.y);
    v = zp(v, zs, blockIdx.y);
    const long long stride = (long long)gridDim.x * kBlock;
    long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x;
    double2 rv[kUnroll], vv[kUnroll];
    auto load = [&]() {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                rv[j] = ld2(r, u);
                vv[j] = ld2(v, u);
            }
        }
    };
    load();                 // the first chunk is in flight while rtv is summed
    const double rtv = sum_partials(part, G);
    const double rho = bs->rho[it & 1];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (bi_bad(rtv)) {
        if (first) {
            bs->bad = rtv;
            bs->why = BI_WHY_RTV;
            bs->done = SR_BREAKDOWN;
        }
        return;
    }
    const double alpha = rho / rtv;
    if (first) bs->alpha = alpha;
    const double na = -alpha;
    while (u0 < units) {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                rv[j].x = na * vv[j].x + rv[j].x;
                rv[j].y = na * vv[j].y + rv[j].y;
                st2(r, u, rv[j]);
            }
        }
        u0 += kUnroll * stride;
        load();
    }
}

// ts, tt from the partials; omega = tt > 0 ? ts / tt : 0 (NaN: 0);
// x = omega s + (alpha p + x);  r = (-omega) t + s in place of s; the block
// partials of r . r (part_out[b]) and rt . r (part_out[G + b]) from the r values
// in registers, each thread's units ascending (k_dot's order)
// SH: the sharded solve -- part_in holds P slots of 2 G doubles (t.s's G, then
// t.t's); the updates run over units (H0 / 2) and the partials over the units
// below dunits (the shard's dot range / 2) alone, so they are bit for bit what
// k_cg_rz gives over the dot range with grid G; part_out is the shard's own 2 G
// slot of a SECOND gathered array -- every block reads all of part_in's array
// while other blocks (and other shards) write part_out's
template <bool SH = false>
__global__ __launch_bounds__(kBlock) void k_bi_xr(Gate g, BiState *bs, const double *part_in, int G,
                                                  double *__restrict__ x, const double *__restrict__ p,
                                                  double *__restrict__ s, const double *__restrict__ t,
                                                  const double *__restrict__ rt, double *part_out,
                                                  long long units, long long zs = 0, int P = 1,
                                                  long long dunits = 0)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    bs = zp(bs, zs, blockIdx.y);
    part_in = zp(part_in, zs, blockIdx.y);
    x = zp(x, zs, blockIdx.y);
    p = zp(p, zs, blockIdx.y);
    s = zp(s, zs, blockIdx.y);
    t = zp(t, zs, blockIdx.y);
    rt = zp(rt, zs, blockIdx.y);
    part_out = zp(part_out, zs, blockIdx.y);
    const long long stride = (long long)gridDim.x * kBlock;
    long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x;
    double2 xv[kUnroll], pv[kUnroll], sv[kUnroll], tv[kUnroll], qv[kUnroll];
    auto load = [&]() {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                xv[j] = ld2(x, u);
                pv[j] = ld2(p, u);
                sv[j] = ld2(s, u);
                tv[j] = ld2(t, u);
                qv[j] = ld2(rt, u);
            }
        }
    };
    load();
    const double ts = SH ? sum_partials_sh(part_in, P, G, 2LL * G) : sum_partials(part_in, G);
    const double tt = SH ? sum_partials_sh(part_in + G, P, G, 2LL * G) : sum_partials(part_in + G, G);
    const double omega = tt > 0.0 ? ts / tt : 0.0;
    const double alpha = bs->alpha;
    if (blockIdx.x == 0 && threadIdx.x == 0) bs->omega = omega;
    const double no = -omega;
    double acc[2] = {0.0, 0.0};
    while (u0 < units) {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                xv[j].x = omega * sv[j].x + (alpha * pv[j].x + xv[j].x);
                xv[j].y = omega * sv[j].y + (alpha * pv[j].y + xv[j].y);
                sv[j].x = no * tv[j].x + sv[j].x;
                sv[j].y = no * tv[j].y + sv[j].y;
                st2(x, u, xv[j]);
                st2(s, u, sv[j]);
                if (!SH || u < dunits) {
                    acc[0] += sv[j].x * sv[j].x;
                    acc[0] += sv[j].y * sv[j].y;
                    acc[1] += qv[j].x * sv[j].x;
                    acc[1] += qv[j].y * sv[j].y;
                }
            }
        }
        u0 += kUnroll * stride;
        load();
    }
    block_sum_store<2>(acc, 2, part_out + blockIdx.x, gridDim.x);
}

// rr, rhon from the partials; res = sqrt(rr) / normb into the history;
// converged (START: res <= tol, else res < tol); else breakdown when omega or
// rhon is zero or not finite (START: rho = rr); otherwise
// p = beta ((-omega) v + p) + r with beta = (rhon / rho) (alpha / omega)
// (START: rt = p = r).  it: the iteration's 0-based index (START: the initial
// residual, nothing counted)
// SH: the sharded solve -- part holds P slots of 2 G doubles (r.r's G, then rt.r's)
template <bool START, bool SH = false>
__global__ __launch_bounds__(kBlock) void k_bi_p(Gate g, int it, BiState *bs, const double *part, int G,
                                                 double *__restrict__ p, const double *__restrict__ v,
                                                 const double *__restrict__ r, double *__restrict__ rt,
                                                 double *hist, long long units, long long zs = 0, int P = 1)
{
    if (gated_z(g, zs, blockIdx.y)) return;
    bs = zp(bs, zs, blockIdx.y);
    part = zp(part, zs, blockIdx.y);
    p = zp(p, zs, blockIdx.y);
    v = zp(v, zs, blockIdx.y);                      // (null at the start: never read there)
    r = zp(r, zs, blockIdx.y);
    rt = zp(rt, zs, blockIdx.y);                    // (null after the start: never written there)
    hist = zp(hist, zs, blockIdx.y);
    const long long stride = (long long)gridDim.x * kBlock;
    long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x;
    double2 pv[kUnroll], vv[kUnroll], rv[kUnroll];
    auto load = [&]() {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                rv[j] = ld2(r, u);
                if (!START) {
                    pv[j] = ld2(p, u);
                    vv[j] = ld2(v, u);
                }
            }
        }
    };
    load();
    const double rr = SH ? sum_partials_sh(part, P, G, 2LL * G) : sum_partials(part, G);
    const double rhon = START ? rr : SH ? sum_partials_sh(part + G, P, G, 2LL * G) : sum_partials(part + G, G);
    const double res = sqrt(rr) / bs->normb;
    const double omega = START ? 1.0 : bs->omega;
    const double alpha = START ? 1.0 : bs->alpha;
    const double rho = START ? 1.0 : bs->rho[it & 1];
    const bool conv = START ? res <= bs->tol : res < bs->tol;
    const bool brk = !conv && (bi_bad(omega) || bi_bad(rhon));
    const int done_it = START ? 0 : it + 1;            // iterations performed
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        bs->resid = res;
        hist[done_it] = res;
        bs->it = done_it;
        bs->rho[done_it & 1] = rhon;
        if (conv) bs->done = START ? SR_INIT : SR_CONV;
        else if (brk) {
            const bool om = bi_bad(omega);
            bs->bad = om ? omega : rhon;
            bs->why = om ? BI_WHY_OMEGA : BI_WHY_RHO;
            bs->done = SR_BREAKDOWN;
        }
    }
    if (conv || brk) return;
    const double beta = (rhon / rho) * (alpha / omega);
    const double no = -omega;
    while (u0 < units) {
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long u = u0 + j * stride;
            if (u < units) {
                if (START) {
                    st2(rt, u, rv[j]);
                } else {
                    rv[j].x = beta * (no * vv[j].x + pv[j].x) + rv[j].x;
                    rv[j].y = beta * (no * vv[j].y + pv[j].y) + rv[j].y;
                }
                st2(p, u, rv[j]);
            }
        }
        u0 += kUnroll * stride;
        load();
    }
}

// the CG batch's control blocks (cg_batch.hip): every scenario's CgState at the
// start of a solve
__global__ void k_init_cg_state_b(CgState *cs, long long zs, int nsc, double tol, int max_iter)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nsc) return;
    CgState h{};
    h.tol = tol;
    h.max_iter = max_iter;
    *zp(cs, zs, q) = h;
}

// the BiCGStab batch's (bicgstab_batch.hip): every scenario's BiState
__global__ void k_init_bi_state_b(BiState *bs, long long zs, int nsc, double tol, int max_iter)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nsc) return;
    BiState h{};
    h.tol = tol;
    h.max_iter = max_iter;
    *zp(bs, zs, q) = h;
}

}  // namespace

// ======================================================= host launchers
// ---- CG (cg.hip) ----------------------------------------------------------------
void launch_init_cg_state_b(CgState *cs, long long zs, int nsc, double tol, int max_iter, hipStream_t st)
{
    k_init_cg_state_b<<<(nsc + 63) / 64, 64, 0, st>>>(cs, zs, nsc, tol, max_iter);
}
void launch_normb(const double *part, int G, double *normb, hipStream_t st, Batch bt)
{
    k_normb<<<dim3(1, bt.nsc), kBlock, 0, st>>>(part, G, normb, bt.zs);
}
void launch_cg_pq(Gate g, const double *p, const double *q, double *part, int G, long long Ppad, hipStream_t st,
                  Batch bt)
{
    k_cg_pq<<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, p, q, part, Ppad / 2, bt.zs);
}
void launch_cg_xr(Gate g, int it, CgState *cs, const double *part, int G, double *x, const double *p, double *r,
                  const double *q, long long Ppad, hipStream_t st, Batch bt)
{
    k_cg_xr<<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, it, cs, part, G, x, p, r, q, Ppad / 2, bt.zs);
}
void launch_cg_rz(Gate g, const double *r, const double *z, double *part, int G, long long Ppad, hipStream_t st,
                  Batch bt)
{
    k_cg_rz<<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, r, z, part, Ppad / 2, bt.zs);
}
void launch_cg_p(Gate g, int it, bool start, CgState *cs, const double *part, int G, double *p, const double *z,
                 double *hist, long long Ppad, hipStream_t st, Batch bt)
{
    if (start) k_cg_p<true><<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, it, cs, part, G, p, z, hist, Ppad / 2, bt.zs);
    else k_cg_p<false><<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, it, cs, part, G, p, z, hist, Ppad / 2, bt.zs);
}
// the sharded solve's consumers (dd.hip): nparts_in = P * G contiguous partials; P slots of 2 G
void launch_cg_xr_r(Gate g, int it, CgState *cs, const double *part, int nparts_in, int G, double *x,
                    const double *p, double *r, const double *q, long long Ppad, hipStream_t st)
{
    k_cg_xr<<<G, kBlock, 0, st>>>(g, it, cs, part, nparts_in, x, p, r, q, Ppad / 2, 0);
}
void launch_cg_p_r(Gate g, int it, bool start, CgState *cs, const double *part, int P, int G, double *p,
                   const double *z, double *hist, long long Ppad, hipStream_t st)
{
    if (start) k_cg_p<true, true><<<G, kBlock, 0, st>>>(g, it, cs, part, G, p, z, hist, Ppad / 2, 0, P);
    else k_cg_p<false, true><<<G, kBlock, 0, st>>>(g, it, cs, part, G, p, z, hist, Ppad / 2, 0, P);
}

// ---- BiCGStab (bicgstab.hip, bicgstab_batch.hip) -----------------------------------
void launch_init_bi_state_b(BiState *bs, long long zs, int nsc, double tol, int max_iter, hipStream_t st)
{
    k_init_bi_state_b<<<(nsc + 63) / 64, 64, 0, st>>>(bs, zs, nsc, tol, max_iter);
}
void launch_bi_s(Gate g, int it, BiState *bs, const double *part, int G, double *r, const double *v,
                 long long Ppad, hipStream_t st, Batch bt)
{
    k_bi_s<<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, it, bs, part, G, r, v, Ppad / 2, bt.zs);
}
void launch_bi_xr(Gate g, BiState *bs, const double *part_in, int G, double *x, const double *p, double *s,
                  const double *t, const double *rt, double *part_out, long long Ppad, hipStream_t st, Batch bt)
{
    k_bi_xr<false><<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, bs, part_in, G, x, p, s, t, rt, part_out, Ppad / 2, bt.zs);
}
void launch_bi_p(Gate g, int it, bool start, BiState *bs, const double *part, int G, double *p, const double *v,
                 const double *r, double *rt, double *hist, long long Ppad, hipStream_t st, Batch bt)
{
    if (start)
        k_bi_p<true><<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, it, bs, part, G, p, v, r, rt, hist, Ppad / 2, bt.zs);
    else
        k_bi_p<false><<<dim3(G, bt.nsc), kBlock, 0, st>>>(g, it, bs, part, G, p, v, r, rt, hist, Ppad / 2, bt.zs);
}
// the sharded solve's consumers (dd.hip): nparts_in = P * G contiguous partials; P slots of 2 G
void launch_bi_s_r(Gate g, int it, BiState *bs, const double *part, int nparts_in, double *r, const double *v,
                   int G, long long Ppad, hipStream_t st)
{
    k_bi_s<<<G, kBlock, 0, st>>>(g, it, bs, part, nparts_in, r, v, Ppad / 2, 0);
}
void launch_bi_xr_r(Gate g, BiState *bs, const double *part_in, int P, int G, double *x, const double *p,
                    double *s, const double *t, const double *rt, double *part_out_slot, long long Ppad,
                    long long dot_len, hipStream_t st)
{
    k_bi_xr<true><<<G, kBlock, 0, st>>>(g, bs, part_in, G, x, p, s, t, rt, part_out_slot, Ppad / 2, 0, P,
                                        dot_len / 2);
}
void launch_bi_p_r(Gate g, int it, bool start, BiState *bs, const double *part, int P, int G, double *p,
                   const double *v, const double *r, double *rt, double *hist, long long Ppad, hipStream_t st)
{
    if (start)
        k_bi_p<true, true><<<G, kBlock, 0, st>>>(g, it, bs, part, G, p, v, r, rt, hist, Ppad / 2, 0, P);
    else
        k_bi_p<false, true><<<G, kBlock, 0, st>>>(g, it, bs, part, G, p, v, r, rt, hist, Ppad / 2, 0, P);
}

}  // namespace gg
