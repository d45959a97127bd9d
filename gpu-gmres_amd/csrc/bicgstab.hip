// bicgstab.hip -- left-preconditioned BiCGStab (GG_SOLVE_BICGSTAB), i.e.
// BiCGStab on (M A) x = M b, on the solver's SpMV, preconditioner and reduction
// tree (DESIGN.md "BiCGStab").
//
//   bb = M b; normb = sqrt(dot(bb, bb));  r = M (b - A x);  res0 = sqrt(dot(r, r)) / normb
//   rt = r;  rho = dot(rt, r);  p = r
//   repeat:  v = M (A p);  rtv = dot(rt, v);  alpha = rho / rtv;  s = (-alpha) v + r
//            t = M (A s);  ts = dot(t, s);  tt = dot(t, t);  omega = tt > 0 ? ts / tt : 0
//            x = omega s + (alpha p + x);  r = (-omega) t + s
//            rr = dot(r, r);  rhon = dot(rt, r);  res = sqrt(rr) / normb
//            beta = (rhon / rho) (alpha / omega);  p = beta ((-omega) v + p) + r;  rho = rhon
//
// The scalars live in the device control block (kernels.h BiState), on which
// every launch of an iteration is gated; the solve around the launches below
// is short_recurrence.h's.  r (and s in its place) = rr, p = w, v = ww,
// x = xv, b = bv from the GMRES work space; the shadow residual, t and the
// SpMV output M is applied to are this solve's own (ensure_vectors).  There is
// no Krylov basis.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "short_recurrence.h"

namespace gg {

namespace {

struct BiCgStab {
    using State = BiState;
    // iterations per chunk: half of CG's, an iteration being twice the launches
    static constexpr int kChunk = 16;
    static constexpr bool kExtraVectors = true;
    static DBuf<State> &control(gg_solver *s) { return s->bis; }
    static void enqueue_start(gg_solver *s);
    static void enqueue_iterations(gg_solver *s, int k0, int k1);
    static std::string breakdown(const State &h)
    {
        const char *name = h.why == BI_WHY_RTV ? "rt.v" : h.why == BI_WHY_OMEGA ? "omega" : "rho";
        char val[40];
        std::snprintf(val, sizeof val, "%g", h.bad);
        return "gg_solve: BiCGStab broke down at iteration " + std::to_string(h.it) + ": " + name + " = " + val +
               " (zero or not finite)";
    }
};

// the three partial arrays (G <= 1024 each) in sr_part: rt.v | t.s, t.t | r.r, rt.r
constexpr int kPartTs = 1024, kPartRr = 3 * 1024;

void BiCgStab::enqueue_start(gg_solver *s)
{
    const Gate none;
    BiState *bs = s->bis.p;
    const long long P = s->Ppad;
    double *part = s->sr_part.p;
    apply_minv(s, none, s->bv.p, s->bb.p);                                  // bb = M b
    launch_dot(none, s->bb.p, s->bb.p, part, s->G, P, s->st);
    launch_normb(part, s->G, &bs->normb, s->st);
    launch_spmv(none, s->dA, s->xv.p, s->bv.p, s->bi_q.p, true, s->st);     // q = b - A x
    apply_minv(s, none, s->bi_q.p, s->rr.p);                                // r = M q
    launch_dot(none, s->rr.p, s->rr.p, part + kPartRr, s->G, P, s->st);
    launch_bi_p(none, 0, true, bs, part + kPartRr, s->G, s->w.p, nullptr, s->rr.p, s->bi_rt.p, s->hist.p, P,
                s->st);                                                     // rt = p = r
}

void BiCgStab::enqueue_iterations(gg_solver *s, int k0, int k1)
{
    BiState *bs = s->bis.p;
    const long long P = s->Ppad;
    double *part = s->sr_part.p;
    double *x = s->xv.p, *r = s->rr.p, *rt = s->bi_rt.p, *p = s->w.p, *v = s->ww.p, *t = s->bi_t.p, *q = s->bi_q.p;
    for (int k = k0; k < k1; k++) {
        Gate g;
        g.done = &bs->done;
        g.mask = ~0;
        g.nit = &bs->max_iter;
        g.i = k;
        int mk = prof_begin(s, GG_PROF_SPMV, k);
        launch_spmv(g, s->dA, p, nullptr, q, false, s->st);                 // q = A p
        prof_end(s, mk);
        mk = prof_begin(s, GG_PROF_PRECOND, k);
        apply_minv(s, g, q, v, k);                                          // v = M q
        prof_end(s, mk);
        launch_cg_pq(g, rt, v, part, s->G, P, s->st);
        launch_bi_s(g, k, bs, part, s->G, r, v, P, s->st);                  // s in place of r
        mk = prof_begin(s, GG_PROF_SPMV, k);
        launch_spmv(g, s->dA, r, nullptr, q, false, s->st);                 // q = A s
        prof_end(s, mk);
        mk = prof_begin(s, GG_PROF_PRECOND, k);
        apply_minv(s, g, q, t, k);                                          // t = M q
        prof_end(s, mk);
        launch_cg_rz(g, r, t, part + kPartTs, s->G, P, s->st);              // s . t, t . t
        launch_bi_xr(g, bs, part + kPartTs, s->G, x, p, r, t, rt, part + kPartRr, P, s->st);
        launch_bi_p(g, k, false, bs, part + kPartRr, s->G, p, v, r, nullptr, s->hist.p, P, s->st);
    }
}

}  // namespace

int solve_bicgstab(gg_solver *s, const double *d_b, double *d_x, const gg_options *opt, gg_result *res)
{
    return solve_short_recurrence<BiCgStab>(s, d_b, d_x, opt, res);
}

}  // namespace gg
