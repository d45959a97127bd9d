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
// The scalars live in the device control block (kernels.h BiState); every
// launch of an iteration is gated on it, so the host enqueues iterations in
// chunks, one chunk ahead of the state it has read, and the launches behind
// the end of the solve do nothing.  r (and s in its place) = rr, p = w, v = ww,
// x = xv, b = bv from the GMRES work space; the shadow residual, t and the
// SpMV output M is applied to are this solve's own (ensure_vectors).  There is
// no Krylov basis.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "kernels.h"
#include "gg_solver.h"

namespace gg {

namespace {

// iterations per chunk: half of CG's, an iteration being twice the launches
constexpr int kChunk = 16;

// the three partial arrays (G <= 1024 each): rt.v | t.s, t.t | r.r, rt.r
constexpr int kPartTs = 1024, kPartRr = 3 * 1024;

void enqueue_start(gg_solver *s)
{
    const Gate none;
    BiState *bs = s->bis.p;
    const long long P = s->Ppad;
    double *part = s->bi_part.p;
    apply_minv(s, none, s->bv.p, s->bb.p);                                  // bb = M b
    launch_dot(none, s->bb.p, s->bb.p, part, s->G, P, s->st);
    launch_bi_normb(part, s->G, bs, s->st);
    launch_spmv(none, s->dA, s->xv.p, s->bv.p, s->bi_q.p, true, s->st);     // q = b - A x
    apply_minv(s, none, s->bi_q.p, s->rr.p);                                // r = M q
    launch_dot(none, s->rr.p, s->rr.p, part + kPartRr, s->G, P, s->st);
    launch_bi_p(none, 0, true, bs, part + kPartRr, s->G, s->w.p, nullptr, s->rr.p, s->bi_rt.p, s->hist.p, P,
                s->st);                                                     // rt = p = r
}

void enqueue_iterations(gg_solver *s, int k0, int k1)
{
    BiState *bs = s->bis.p;
    const long long P = s->Ppad;
    double *part = s->bi_part.p;
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

void bicgstab_release(gg_solver *s)
{
    for (int k = 0; k < 2; k++) {
        if (s->bi_state[k]) (void)hipHostFree(s->bi_state[k]);
        if (s->bi_err[k]) (void)hipHostFree(s->bi_err[k]);
        if (s->bi_ev[k]) (void)hipEventDestroy(s->bi_ev[k]);
        s->bi_state[k] = nullptr;
        s->bi_err[k] = nullptr;
        s->bi_ev[k] = nullptr;
    }
}

int solve_bicgstab(gg_solver *s, const double *d_b, double *d_x, const gg_options *opt, gg_result *res)
{
    const int n = s->A.n;
    const int max_iter = opt->max_iter;
    ensure_vectors(s, true);
    if (!s->bis.p) s->bis.alloc(1);
    if (!s->bi_part.p) s->bi_part.alloc(5 * 1024);
    const long long need = (long long)max_iter + 1;
    if (need > s->hist_cap) {
        s->hist.alloc(need);
        s->hist_cap = need;
    }
    for (int k = 0; k < 2; k++)
        if (!s->bi_state[k]) {
            GG_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->bi_state[k]), sizeof(BiState), hipHostMallocDefault));
            GG_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->bi_err[k]), sizeof(int), hipHostMallocDefault));
            GG_HIP(hipEventCreateWithFlags(&s->bi_ev[k], hipEventDisableTiming));
        }
    launch_gather(d_b, s->lay2nat.p, s->bv.p, s->Ppad, s->st);
    launch_gather(d_x, s->lay2nat.p, s->xv.p, s->Ppad, s->st);
    for (DevTri *T : {&s->L, &s->U})
        if (T->kind == DevTri::WAVE2D) reset_wave(T, s->st);
    BiState h0{};
    h0.tol = opt->tol;
    h0.max_iter = max_iter;
    GG_HIP(hipMemcpyAsync(s->bis.p, &h0, sizeof(BiState), hipMemcpyHostToDevice, s->st));
    GG_HIP(hipMemsetAsync(s->err.p, 0, sizeof(int), s->st));

    GG_HIP(hipEventRecord(s->ev0, s->st));
    enqueue_start(s);
    // chunks of iterations, the host one chunk ahead (cg.hip's loop): chunk c + 1
    // goes in before the state after chunk c is read.  In a transient the first
    // chunk is the previous step's count + 2 (solver.hip iter_hint)
    std::vector<size_t> mark_ends;
    int next = 0;                                       // first iteration not yet enqueued
    auto enqueue = [&](int slot, int len) {
        const int k1 = (int)std::min<long long>((long long)next + len, max_iter);
        enqueue_iterations(s, next, k1);
        next = k1;
        mark_ends.push_back(s->marks.size());
        GG_HIP(hipMemcpyAsync(s->bi_state[slot], s->bis.p, sizeof(BiState), hipMemcpyDeviceToHost, s->st));
        GG_HIP(hipMemcpyAsync(s->bi_err[slot], s->err.p, sizeof(int), hipMemcpyDeviceToHost, s->st));
        GG_HIP(hipEventRecord(s->bi_ev[slot], s->st));
    };
    auto collect = [&](int executed) {                  // the oldest enqueued chunk's marks
        const size_t upto = mark_ends.empty() ? s->marks.size() : mark_ends.front();
        prof_collect(s, executed, upto);
        if (!mark_ends.empty()) {
            mark_ends.erase(mark_ends.begin());
            for (size_t &e : mark_ends) e -= upto;
        }
    };
    auto drain = [&]() {                                // the chunk behind the last (gated off)
        GG_HIP(hipStreamSynchronize(s->st));
        while (!mark_ends.empty()) collect(0);
        prof_collect(s, 0);
    };
    enqueue(0, s->iter_hint > 0 ? s->iter_hint + 2 : kChunk);
    enqueue(1, kChunk);
    int cur = 0;
    BiState h{};
    while (true) {
        GG_HIP(hipEventSynchronize(s->bi_ev[cur]));
        const int err = *s->bi_err[cur];
        h = *s->bi_state[cur];
        if (err & (8 | 2)) {
            drain();
            throw Fallback{err};
        }
        if (err & 1) {
            drain();
            GG_REQUIRE(false, GG_ETIMEOUT, "wavefront triangular solve: boundary wait timed out");
        }
        collect(h.it);                                  // marks of completed iterations count
        if (h.done || h.it >= max_iter) break;
        enqueue(cur, kChunk);
        cur ^= 1;
    }
    drain();
    GG_HIP(hipEventRecord(s->ev1, s->st));
    check_err(s);
    launch_gather(s->xv.p, s->nat2lay.p, d_x, n, s->st);
    GG_HIP(hipStreamSynchronize(s->st));
    float ms = 0.f;
    GG_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    const long long hist_len = (long long)h.it + 1;
    s->last_hist.resize(hist_len);
    GG_HIP(hipMemcpy(s->last_hist.data(), s->hist.p, hist_len * sizeof(double), hipMemcpyDeviceToHost));
    int ret = GG_NOT_CONVERGED;
    if (h.done & (BI_CONV | BI_INIT)) ret = GG_OK;
    else if (h.done & BI_BREAKDOWN) {
        ret = GG_EBREAKDOWN;
        const char *name = h.why == BI_WHY_RTV ? "rt.v" : h.why == BI_WHY_OMEGA ? "omega" : "rho";
        char val[40];
        std::snprintf(val, sizeof val, "%g", h.bad);
        set_error("gg_solve: BiCGStab broke down at iteration " + std::to_string(h.it) + ": " + name + " = " +
                  val + " (zero or not finite)");
    }
    if (res) {
        res->status = ret;
        res->iters = h.it;
        res->inner_iters = h.it;
        res->restarts = 0;
        res->relres = h.resid;
        res->solve_ms = ms;
    }
    return ret;
}

}  // namespace gg
