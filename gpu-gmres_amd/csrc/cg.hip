// cg.hip -- left-preconditioned conjugate gradients (GG_SOLVE_CG) on the
// solver's SpMV, preconditioner and reduction tree (DESIGN.md "CG").
//
//   bb = M b; normb = sqrt(dot(bb, bb));  r = b - A x;  z = M r
//   res0 = sqrt(dot(z, z)) / normb;  p = z;  rz = dot(r, z)
//   repeat:  q = A p;  pq = dot(p, q);  alpha = rz / pq
//            x = alpha p + x;  r = (-alpha) q + r
//            z = M r;  rzn = dot(r, z);  zz = dot(z, z);  res = sqrt(zz) / normb
//            beta = rzn / rz;  p = beta p + z;  rz = rzn
//
// The scalars live in the device control block (kernels.h CgState), on which
// every launch of an iteration is gated; the solve around the launches below
// is short_recurrence.h's.  Vectors reuse the solver's work space (r = rr,
// z = r, p = w, q = ww, x = xv, b = bv); there is no Krylov basis.
#include <hip/hip_runtime.h>

#include <string>

#include "short_recurrence.h"

namespace gg {

namespace {

struct Cg {
    using State = CgState;
    // iterations per chunk: a host round trip is hidden behind the chunk in
    // flight, a converged solve runs at most two chunks of launches that read
    // their gate and return
    static constexpr int kChunk = 32;
    static constexpr bool kExtraVectors = false;
    static DBuf<State> &control(gg_solver *s) { return s->cgs; }
    static void enqueue_start(gg_solver *s);
    static void enqueue_iterations(gg_solver *s, int k0, int k1);
    static std::string breakdown(const State &h)
    {
        return "gg_solve: conjugate gradients broke down at iteration " + std::to_string(h.it) +
               " (p.Ap or r.Mr not positive: A and M must be symmetric positive definite)";
    }
};

// the partial arrays (G <= 1024 each) in sr_part: p.q | r.z, z.z
void Cg::enqueue_start(gg_solver *s)
{
    const Gate none;
    CgState *cs = s->cgs.p;
    const long long P = s->Ppad;
    double *part = s->sr_part.p;
    apply_minv(s, none, s->bv.p, s->bb.p);                                  // bb = M b
    launch_dot(none, s->bb.p, s->bb.p, part, s->G, P, s->st);
    launch_normb(part, s->G, &cs->normb, s->st);
    launch_spmv(none, s->dA, s->xv.p, s->bv.p, s->rr.p, true, s->st);       // r = b - A x
    apply_minv(s, none, s->rr.p, s->r.p);                                   // z = M r
    launch_cg_rz(none, s->rr.p, s->r.p, part + 1024, s->G, P, s->st);
    launch_cg_p(none, 0, true, cs, part + 1024, s->G, s->w.p, s->r.p, s->hist.p, P, s->st);   // p = z
}

void Cg::enqueue_iterations(gg_solver *s, int k0, int k1)
{
    CgState *cs = s->cgs.p;
    const long long P = s->Ppad;
    double *part = s->sr_part.p;
    double *x = s->xv.p, *r = s->rr.p, *z = s->r.p, *p = s->w.p, *q = s->ww.p;
    for (int k = k0; k < k1; k++) {
        Gate g;
        g.done = &cs->done;
        g.mask = ~0;
        g.nit = &cs->max_iter;
        g.i = k;
        int mk = prof_begin(s, GG_PROF_SPMV, k);
        launch_spmv(g, s->dA, p, nullptr, q, false, s->st);                 // q = A p
        prof_end(s, mk);
        launch_cg_pq(g, p, q, part, s->G, P, s->st);
        launch_cg_xr(g, k, cs, part, s->G, x, p, r, q, P, s->st);
        mk = prof_begin(s, GG_PROF_PRECOND, k);
        apply_minv(s, g, r, z, k);                                          // z = M r
        prof_end(s, mk);
        launch_cg_rz(g, r, z, part + 1024, s->G, P, s->st);
        launch_cg_p(g, k, false, cs, part + 1024, s->G, p, z, s->hist.p, P, s->st);
    }
}

}  // namespace

int solve_cg(gg_solver *s, const double *d_b, double *d_x, const gg_options *opt, gg_result *res)
{
    return solve_short_recurrence<Cg>(s, d_b, d_x, opt, res);
}

}  // namespace gg
