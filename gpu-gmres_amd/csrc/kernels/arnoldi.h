// kernels/arnoldi.h -- the Givens update of a Hessenberg column, shared by the per-step orthogonalization
// kernels (kernels.hip) and the one-launch ones (kernels/arnoldi_persist.hip).
#pragma once

#include "device.h"

namespace gg {

namespace {

__device__ __forceinline__ void apply_rot(double &dx, double &dy, double cs, double sn)
{
    double temp = cs * dx + sn * dy;     // ApplyPlaneRotation (src/gmres.cu:192-197)
    dy = -sn * dx + cs * dy;
    dx = temp;
}
__device__ __forceinline__ void gen_rot(double dx, double dy, double &cs, double &sn)
{
    if (dy == 0.0) { cs = 1.0; sn = 0.0; }   // GeneratePlaneRotation (:200-216)
    else if (fabs(dy) > fabs(dx)) {
        double temp = dx / dy;
        sn = 1.0 / sqrt(1.0 + temp * temp);
        cs = temp * sn;
    } else {
        double temp = dy / dx;
        cs = 1.0 / sqrt(1.0 + temp * temp);
        sn = temp * cs;
    }
}

// ---- the Givens update of Hessenberg column i, written once -------------------
// The reference's sequence -- apply_rot(Hc[k], Hc[k+1], cs[k], sn[k]) for k < i,
// gen_rot, the two last apply_rot, the residual test -- as a pair of steps that
// keep the column on chip: `lo` is Hc[k] with rotations 0..k-1 applied, the one
// entry the next rotation still needs.  The same calls on the same operands in
// the same order as the loop over memory, so the same bits; what changes is
// that no rotation waits for the previous one's stores and its own loads.
//
// givens_absorb: h_{k+1} is known -- rotation k on (Hc[k], h_{k+1}); returns the
// final Hc[k], keeps the rotated Hc[k+1]
__device__ __forceinline__ double givens_absorb(double &lo, double hnext, double c, double s)
{
    apply_rot(lo, hnext, c, s);
    const double fin = lo;
    lo = hnext;
    return fin;
}
// what the column's last step reads besides the column: loaded up front
struct GivensIn {
    double si, si1, normb, tol;
    int hist_len;
};
__device__ __forceinline__ GivensIn givens_load(const double *s, const DevState *ds, int i)
{
    GivensIn in;
    in.si = s[i];
    in.si1 = s[i + 1];
    in.normb = ds->normb;
    in.tol = ds->tol;
    in.hist_len = ds->hist_len;
    return in;
}
// givens_finish: lo = Hc[i] (rotations 0..i-1 applied), hn = ||w||: the new
// rotation on the column and on s, the residual, the history entry and the
// convergence flag -- arithmetic on registers, then stores
struct GivensOut {
    double c, s, resid;
};
__device__ __forceinline__ GivensOut givens_finish(double lo, double hn, const GivensIn &in, int i, double *Hc,
                                                   double *cs, double *sn, double *s, double *hist, DevState *ds)
{
    double hi = lo, hi1 = hn, c, sv;
    gen_rot(hi, hi1, c, sv);
    apply_rot(hi, hi1, c, sv);
    double si = in.si, si1 = in.si1;
    apply_rot(si, si1, c, sv);
    const double resid = fabs(si1) / in.normb;
    Hc[i] = hi;
    Hc[i + 1] = hi1;
    cs[i] = c;
    sn[i] = sv;
    s[i] = si;
    s[i + 1] = si1;
    hist[in.hist_len + i] = resid;
    ds->resid = resid;
    if (resid < in.tol) {                // "<" (src/gmres.cu:654)
        ds->conv_i = i;
        ds->done = DONE_INNER;
    }
    return {c, sv, resid};
}
// the whole column from memory (the per-step kernels' finalize): Hc[0..i] hold
// the raw h_k.  The inputs of kGivensBatch rotations are loaded together, and
// every load of the last step goes out before the first rotation, so the chain
// is one memory latency per batch instead of one per rotation.
constexpr int kGivensBatch = 8;
__device__ __forceinline__ void givens_column(int i, double hn, double *Hc, double *cs, double *sn, double *s,
                                              double *hist, DevState *ds)
{
    const GivensIn in = givens_load(s, ds, i);
    double lo = Hc[0];
    for (int k0 = 0; k0 < i; k0 += kGivensBatch) {
        double h[kGivensBatch], c[kGivensBatch], r[kGivensBatch];
#pragma unroll
        for (int q = 0; q < kGivensBatch; q++) {
            const int k = k0 + q < i ? k0 + q : i - 1;      // (the tail repeats a valid entry, unused)
            h[q] = Hc[k + 1];
            c[q] = cs[k];
            r[q] = sn[k];
        }
#pragma unroll
        for (int q = 0; q < kGivensBatch; q++)
            if (k0 + q < i) Hc[k0 + q] = givens_absorb(lo, h[q], c[q], r[q]);
    }
    givens_finish(lo, hn, in, i, Hc, cs, sn, s, hist, ds);
}

}  // namespace

}  // namespace gg
