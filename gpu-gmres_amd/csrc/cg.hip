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
// The scalars live in the device control block (kernels.h CgState); every
// launch of an iteration is gated on it, so the host enqueues iterations in
// chunks, one chunk ahead of the state it has read, and the launches behind
// the end of the solve do nothing.  Vectors reuse the solver's work space
// (r = rr, z = r, p = w, q = ww, x = xv, b = bv); there is no Krylov basis.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "kernels.h"
#include "gg_solver.h"

namespace gg {

namespace {

// iterations per chunk: a host round trip is hidden behind the chunk in
// flight, a converged solve runs at most two chunks of launches that read
// their gate and return
constexpr int kChunk = 32;

void enqueue_start(gg_solver *s)
{
    const Gate none;
    CgState *cs = s->cgs.p;
    const long long P = s->Ppad;
    double *part = s->cg_part.p;
    apply_minv(s, none, s->bv.p, s->bb.p);                                  // bb = M b
    launch_dot(none, s->bb.p, s->bb.p, part, s->G, P, s->st);
    launch_cg_normb(part, s->G, cs, s->st);
    launch_spmv(none, s->dA, s->xv.p, s->bv.p, s->rr.p, true, s->st);       // r = b - A x
    apply_minv(s, none, s->rr.p, s->r.p);                                   // z = M r
    launch_cg_rz(none, s->rr.p, s->r.p, part + 1024, s->G, P, s->st);
    launch_cg_p(none, 0, true, cs, part + 1024, s->G, s->w.p, s->r.p, s->hist.p, P, s->st);   // p = z
}

void enqueue_iterations(gg_solver *s, int k0, int k1)
{
    CgState *cs = s->cgs.p;
    const long long P = s->Ppad;
    double *part = s->cg_part.p;
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

void cg_release(gg_solver *s)
{
    for (int k = 0; k < 2; k++) {
        if (s->cg_state[k]) (void)hipHostFree(s->cg_state[k]);
        if (s->cg_err[k]) (void)hipHostFree(s->cg_err[k]);
        if (s->cg_ev[k]) (void)hipEventDestroy(s->cg_ev[k]);
        s->cg_state[k] = nullptr;
        s->cg_err[k] = nullptr;
        s->cg_ev[k] = nullptr;
    }
}

int solve_cg(gg_solver *s, const double *d_b, double *d_x, const gg_options *opt, gg_result *res)
{
    const int n = s->A.n;
    const int max_iter = opt->max_iter;
    ensure_vectors(s);
    if (!s->cgs.p) s->cgs.alloc(1);
    if (!s->cg_part.p) s->cg_part.alloc(3 * 1024);     // p.q | r.z, z.z (G <= 1024 each)
    const long long need = (long long)max_iter + 1;
    if (need > s->hist_cap) {
        s->hist.alloc(need);
        s->hist_cap = need;
    }
    for (int k = 0; k < 2; k++)
        if (!s->cg_state[k]) {
            GG_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->cg_state[k]), sizeof(CgState), hipHostMallocDefault));
            GG_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->cg_err[k]), sizeof(int), hipHostMallocDefault));
            GG_HIP(hipEventCreateWithFlags(&s->cg_ev[k], hipEventDisableTiming));
        }
    launch_gather(d_b, s->lay2nat.p, s->bv.p, s->Ppad, s->st);
    launch_gather(d_x, s->lay2nat.p, s->xv.p, s->Ppad, s->st);
    for (DevTri *T : {&s->L, &s->U})
        if (T->kind == DevTri::WAVE2D) reset_wave(T, s->st);
    CgState h0{};
    h0.tol = opt->tol;
    h0.max_iter = max_iter;
    GG_HIP(hipMemcpyAsync(s->cgs.p, &h0, sizeof(CgState), hipMemcpyHostToDevice, s->st));
    GG_HIP(hipMemsetAsync(s->err.p, 0, sizeof(int), s->st));

    GG_HIP(hipEventRecord(s->ev0, s->st));
    enqueue_start(s);
    // chunks of iterations, the host one chunk ahead: chunk c + 1 goes in before
    // the state after chunk c is read.  In a transient the first chunk is the
    // previous step's count + 2 (solver.hip iter_hint), so a step that converges
    // as its predecessor did enqueues little behind its end
    std::vector<size_t> mark_ends;
    int next = 0;                                       // first iteration not yet enqueued
    auto enqueue = [&](int slot, int len) {
        const int k1 = (int)std::min<long long>((long long)next + len, max_iter);
        enqueue_iterations(s, next, k1);
        next = k1;
        mark_ends.push_back(s->marks.size());
        GG_HIP(hipMemcpyAsync(s->cg_state[slot], s->cgs.p, sizeof(CgState), hipMemcpyDeviceToHost, s->st));
        GG_HIP(hipMemcpyAsync(s->cg_err[slot], s->err.p, sizeof(int), hipMemcpyDeviceToHost, s->st));
        GG_HIP(hipEventRecord(s->cg_ev[slot], s->st));
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
    CgState h{};
    while (true) {
        GG_HIP(hipEventSynchronize(s->cg_ev[cur]));
        const int err = *s->cg_err[cur];
        h = *s->cg_state[cur];
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
    if (h.done & (CG_CONV | CG_INIT)) ret = GG_OK;
    else if (h.done & CG_BREAKDOWN) {
        ret = GG_EBREAKDOWN;
        set_error("gg_solve: conjugate gradients broke down at iteration " + std::to_string(h.it) +
                  " (p.Ap or r.Mr not positive: A and M must be symmetric positive definite)");
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
