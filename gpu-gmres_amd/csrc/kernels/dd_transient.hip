// dd_transient.hip -- the per-step kernels of the sharded transient loop (dd.hip "Sharded
// transient"): a shard's right-hand side formed in its slots, and the port capture.
#include "device.h"
#include "host.h"

namespace gg {

namespace {

// One slot of w = B u + (C/h) x: k_transient_rhs's operations in its order (kernels.hip:
// w = 0; w += B u with the row's sources in ascending k; xnr = 0; xnr += (C/h) x; w += xnr),
// so a row's value is bit-identical to the natural-order kernel's.  A padding slot has no
// sources and c = x = +0.0 there: 0.0 + (0.0 + 0.0 * 0.0) = +0.0.
__device__ __forceinline__ double rhs_slot(int q0, int q1, const int *__restrict__ sidx,
                                           const double *__restrict__ u, double c, double x)
{
    double bu = 0.0;
    for (int q = q0; q < q1; q++) bu = bu + 1.0 * u[sidx[q]];
    double xnr = 0.0;
    xnr = xnr + c * x;
    return bu + xnr;
}

// b[0, 2 * units) = B u + (C/h) x over a shard's slots [0, H0): thread t takes the 16-B
// units t, t + stride, .. with kUnroll units' loads in flight (x and c as double2, the
// unit's two source pointers as one int2 and the third from the next unit's line); the
// per-slot source loop is almost always empty.  Reads x, writes b, nothing past H0 (the
// halo belongs to the exchanges); one writer per output, plain loads and stores.
__global__ __launch_bounds__(kBlock) void k_dd_transient_rhs(const int *__restrict__ sptr,
                                                             const int *__restrict__ sidx,
                                                             const double *__restrict__ u,
                                                             const double *__restrict__ c,
                                                             const double *__restrict__ x, double *__restrict__ b,
                                                             long long units)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u0 = blockIdx.x * (long long)kBlock + threadIdx.x; u0 < units; u0 += kUnroll * stride) {
        double2 xv[kUnroll], cv[kUnroll];
        int2 p[kUnroll];
        int pe[kUnroll];
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long un = u0 + j * stride;
            if (un < units) {
                xv[j] = ld2(x, un);
                cv[j] = ld2(c, un);
                p[j] = reinterpret_cast<const int2 *>(sptr)[un];
                pe[j] = sptr[2 * un + 2];
            }
        }
#pragma unroll
        for (int j = 0; j < kUnroll; j++) {
            const long long un = u0 + j * stride;
            if (un < units) {
                double2 w;
                w.x = rhs_slot(p[j].x, p[j].y, sidx, u, cv[j].x, xv[j].x);
                w.y = rhs_slot(p[j].y, pe[j], sidx, u, cv[j].y, xv[j].y);
                st2(b, un, w);
            }
        }
    }
}

// out[j] = the held port j's value: xv.p[psh[j]][pslot[j]] (psh[j] < 0: not held by this
// process, out[j] keeps its value)
__global__ void k_dd_ports(int nport, const int *__restrict__ psh, const long long *__restrict__ pslot,
                           ShardPtrs xv, double *__restrict__ out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nport) return;
    const int k = psh[j];
    if (k >= 0) out[j] = xv.p[k][pslot[j]];
}

}  // namespace

void launch_dd_transient_rhs(const int *sptr, const int *sidx, const double *u, const double *c, const double *x,
                             double *b, long long H0, hipStream_t st)
{
    const long long units = H0 / 2;
    if (units <= 0) return;
    k_dd_transient_rhs<<<blocks_for((units + kUnroll - 1) / kUnroll, kBlock, 2048), kBlock, 0, st>>>(sptr, sidx, u, c,
                                                                                                    x, b, units);
}

void launch_dd_ports(int nport, const int *psh, const long long *pslot, const ShardPtrs &xv, double *out,
                     hipStream_t st)
{
    if (nport > 0) k_dd_ports<<<(nport + kBlock - 1) / kBlock, kBlock, 0, st>>>(nport, psh, pslot, xv, out);
}

}  // namespace gg
