// short_recurrence.h -- the solve that the short-recurrence Krylov methods
// (cg.hip, bicgstab.hip) share, written once over a method description.
//
// A method keeps its scalars in a device control block and gates every launch
// of an iteration on it, so the host enqueues iterations in chunks, one chunk
// ahead of the state it has read (gg_solver.h ReadPipe), and the launches
// behind the end of the solve do nothing.  The description M supplies
//   State                      the control block (kernels.h), with members done
//                              (SR_* bits), it, resid, tol, max_iter
//   kChunk                     iterations per chunk
//   kExtraVectors              whether it needs BiCGStab's three vectors (ensure_vectors)
//   control(s)                 the DBuf<State> on the solver
//   enqueue_start(s)           normb, the initial residual, hist[0], the first direction
//   enqueue_iterations(s, k0, k1)
//   breakdown(h)               the message for SR_BREAKDOWN, from a host copy of the state
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "kernels.h"
#include "gg_solver.h"

namespace gg {

template <class M>
int solve_short_recurrence(gg_solver *s, const double *d_b, double *d_x, const gg_options *opt, gg_result *res)
{
    using State = typename M::State;
    const int n = s->A.n;
    const int max_iter = opt->max_iter;
    ensure_vectors(s, M::kExtraVectors);
    DBuf<State> &ctl = M::control(s);
    if (!ctl.p) ctl.alloc(1);
    if (!s->sr_part.p) s->sr_part.alloc(5 * 1024);     // BiCGStab's five arrays of G <= 1024 partials; CG uses three
    const long long need = (long long)max_iter + 1;
    if (need > s->hist_cap) {
        s->hist.alloc(need);
        s->hist_cap = need;
    }
    pipe_begin(s);
    launch_gather(d_b, s->lay2nat.p, s->bv.p, s->Ppad, s->st);
    launch_gather(d_x, s->lay2nat.p, s->xv.p, s->Ppad, s->st);
    for (DevTri *T : {&s->L, &s->U})
        if (T->kind == DevTri::WAVE2D) reset_wave(T, s->st);
    State h0{};
    h0.tol = opt->tol;
    h0.max_iter = max_iter;
    GG_HIP(hipMemcpyAsync(ctl.p, &h0, sizeof(State), hipMemcpyHostToDevice, s->st));
    GG_HIP(hipMemsetAsync(s->err.p, 0, sizeof(int), s->st));

    GG_HIP(hipEventRecord(s->ev0, s->st));
    M::enqueue_start(s);
    // chunks of iterations, the host one chunk ahead: chunk c + 1 goes in before
    // the state after chunk c is read.  In a transient the first chunk is the
    // previous step's count + 2 (solver.hip iter_hint), so a step that converges
    // as its predecessor did enqueues little behind its end
    int next = 0;                                       // first iteration not yet enqueued
    auto enqueue = [&](int slot, int len) {
        const int k1 = (int)std::min<long long>((long long)next + len, max_iter);
        M::enqueue_iterations(s, next, k1);
        next = k1;
        pipe_post(s, slot, ctl.p, sizeof(State));
    };
    enqueue(0, s->iter_hint > 0 ? s->iter_hint + 2 : M::kChunk);
    enqueue(1, M::kChunk);
    int cur = 0;
    State h{};
    while (true) {
        const int err = pipe_wait(s, cur);
        h = pipe_state<State>(s, cur);
        if (err & kErrSolve) {
            pipe_drain(s);
            raise_err(err);
        }
        pipe_collect(s, h.it);                          // marks of completed iterations count
        if (h.done || h.it >= max_iter) break;
        enqueue(cur, M::kChunk);
        cur ^= 1;
    }
    pipe_drain(s);
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
    if (h.done & (SR_CONV | SR_INIT)) ret = GG_OK;
    else if (h.done & SR_BREAKDOWN) {
        ret = GG_EBREAKDOWN;
        set_error(M::breakdown(h));
        // the scalar may not have been finite: NaN in the vectors' padding would
        // reach every dot of the next solve on this solver
        zero_vectors(s);
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
