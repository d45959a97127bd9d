// bicgstab_batch.hip -- the many-RHS BiCGStab solve: nrhs independent
// right-hand sides on ONE matrix and preconditioner, every launch of a
// BiCGStab iteration serving all scenarios (DESIGN.md "BiCGStab batch").
//
// The method is bicgstab.hip's, the batch is cg_batch.hip's: scenario q keeps
// its own vectors, partials, control block (BiState) and history in an arena of
// its own, q * zs bytes after scenario 0's, and an iteration is eleven launches
// for all scenarios together --
//   launch_spmv_b        q = A p      (A's entries read once per 8 scenarios)
//   launch_trsv_b L, U   v = M q      (one wavefront dependency chain for all)
//   launch_cg_pq         partials of rt . v
//   launch_bi_s          alpha; s = (-alpha) v + r in place of r
//   launch_spmv_b        q = A s
//   launch_trsv_b L, U   t = M q
//   launch_cg_rz         partials of t . s and t . t
//   launch_bi_xr         omega; x, r; partials of r . r and rt . r
//   launch_bi_p          res, beta; p = beta ((-omega) v + p) + r
// Per scenario the arithmetic is the single solve's -- the same kernels with a
// scenario offset -- so scenario q's status, count, history and solution are
// bit-identical to gg_solve_device(GG_SOLVE_BICGSTAB) on that right-hand side
// alone.  A scenario whose gate is closed (converged, converged at the start,
// broken down, max_iter reached) drops out of every launch; the others go on.
//
// Iterations are enqueued in chunks with the host one chunk ahead of the
// control blocks it has read (batch_common.h's ReadRing, as the CG batch); there
// is no host synchronization per iteration.  The batch ends when a read-back
// shows every scenario over; the launches enqueued behind that point are gated
// off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "batch_common.h"

namespace gg {

// The work space: the arena and read-back ring (batch_common.h), scenario 0's
// arrays in the arena, and the histories of a scenario-by-scenario run.
struct BiBatchWs {
    BatchArena arena;                    // (no method key: 0)
    ReadRing<BiState> ring;
    BiState *bs = nullptr;
    // the vectors are taken first and side by side: [x, part) is what a
    // scenario that broke down gets zeroed (rezero)
    double *x = nullptr, *b = nullptr, *r = nullptr, *rt = nullptr, *p = nullptr, *v = nullptr, *t = nullptr,
           *q = nullptr, *bb = nullptr, *t1 = nullptr, *part = nullptr, *hist = nullptr;
    // the last solve's histories: arena.hist_len (batched), or the vectors
    // themselves (scenario by scenario)
    bool seq = false;
    std::vector<std::vector<double>> seq_hist;
};

void bicgstab_batch_release(gg_solver *s)
{
    delete s->bi_batch;
    s->bi_batch = nullptr;
}

namespace {

// Iterations per chunk after the first.  A BiCGStab iteration is eleven
// dispatches for all scenarios where a CG iteration is seven, and a batch that
// is over leaves up to two chunks of launches that read their gates and
// return, so the chunk is half of the CG batch's 8 (DESIGN.md "BiCGStab
// batch").  It changes no bits.
constexpr int kBiBatchChunk = 4;

// the partial arrays (G <= 1024 each) in part, as bicgstab.hip: rt.v | t.s, t.t | r.r, rt.r
constexpr int kPartTs = 1024, kPartRr = 3 * 1024;

BiBatchWs *ws(gg_solver *s)
{
    if (!s->bi_batch) s->bi_batch = new BiBatchWs;
    return s->bi_batch;
}

void ensure_bi_batch(gg_solver *s, int S, long long hist_need)
{
    BiBatchWs *B = ws(s);
    BatchArena &A = B->arena;
    if (A.fits(s, S, hist_need, 0)) return;
    A.begin(s, S, hist_need, 0);
    const long long P = s->Ppad;
    A.take(B->x, P);
    A.take(B->b, P);
    A.take(B->r, P);
    A.take(B->rt, P);
    A.take(B->p, P);
    A.take(B->v, P);
    A.take(B->t, P);
    A.take(B->q, P);
    A.take(B->bb, P);
    A.take(B->t1, P);
    A.take(B->part, 5 * 1024);
    A.take(B->bs, 1);
    A.take(B->hist, A.hist_cap);
    A.take(A.Lg, A.ngL);
    A.take(A.Ug, A.ngU);
    A.commit(s->st);
    B->ring.alloc(S);
}

struct Ctx {
    gg_solver *s;
    BiBatchWs *B;
    int S, G;
    long long P, zs;
};

// BiCgStab::enqueue_start for every scenario
void enqueue_start_b(const Ctx &c)
{
    gg_solver *s = c.s;
    const BiBatchWs &a = *c.B;
    const Gate none;
    const Batch bt{c.S, c.zs};
    batch_minv(s, a.arena, none, a.b, a.t1, a.bb);                                  // bb = M b
    launch_dot(none, a.bb, a.bb, a.part, c.G, c.P, s->st, bt);
    launch_normb(a.part, c.G, &a.bs->normb, s->st, bt);
    launch_spmv_b(none, s->dA, a.x, a.b, a.q, true, c.S, c.zs, s->st);              // q = b - A x
    batch_minv(s, a.arena, none, a.q, a.t1, a.r);                                   // r = M q
    launch_dot(none, a.r, a.r, a.part + kPartRr, c.G, c.P, s->st, bt);
    launch_bi_p(none, 0, true, a.bs, a.part + kPartRr, c.G, a.p, nullptr, a.r, a.rt, a.hist, c.P, s->st,
                bt);                                                                // rt = p = r
}

// BiCgStab::enqueue_iterations for every scenario, each launch gated per scenario
void enqueue_iterations_b(const Ctx &c, int k0, int k1)
{
    gg_solver *s = c.s;
    const BiBatchWs &a = *c.B;
    const Batch bt{c.S, c.zs};
    for (int k = k0; k < k1; k++) {
        Gate g;
        g.done = &a.bs->done;
        g.mask = ~0;
        g.nit = &a.bs->max_iter;
        g.i = k;
        launch_spmv_b(g, s->dA, a.p, nullptr, a.q, false, c.S, c.zs, s->st);        // q = A p
        batch_minv(s, a.arena, g, a.q, a.t1, a.v);                                  // v = M q
        launch_cg_pq(g, a.rt, a.v, a.part, c.G, c.P, s->st, bt);
        launch_bi_s(g, k, a.bs, a.part, c.G, a.r, a.v, c.P, s->st, bt);             // s in place of r
        launch_spmv_b(g, s->dA, a.r, nullptr, a.q, false, c.S, c.zs, s->st);        // q = A s
        batch_minv(s, a.arena, g, a.q, a.t1, a.t);                                  // t = M q
        launch_cg_rz(g, a.r, a.t, a.part + kPartTs, c.G, c.P, s->st, bt);           // s . t, t . t
        launch_bi_xr(g, a.bs, a.part + kPartTs, c.G, a.x, a.p, a.r, a.t, a.rt, a.part + kPartRr, c.P, s->st, bt);
        launch_bi_p(g, k, false, a.bs, a.part + kPartRr, c.G, a.p, a.v, a.r, nullptr, a.hist, c.P, s->st, bt);
    }
}

// one scenario's outcome and, after a breakdown, the scalar that caused it
struct Outcome {
    gg_result r{};
    int why = 0;
    double bad = 0.0;
};

std::string breakdown_msg(int q, const Outcome &o)
{
    const char *name = o.why == BI_WHY_RTV ? "rt.v" : o.why == BI_WHY_OMEGA ? "omega" : "rho";
    char val[40];
    std::snprintf(val, sizeof val, "%g", o.bad);
    return "gg_solve_bicgstab_batch: BiCGStab broke down in scenario " + std::to_string(q) + " at iteration " +
           std::to_string(o.r.iters) + ": " + name + " = " + val + " (zero or not finite)";
}

// what a batch returns from its scenarios' statuses
int batch_status(int S, const std::vector<Outcome> &o)
{
    int rc = GG_OK;
    for (int q = S - 1; q >= 0; q--) {
        if (o[q].r.status == GG_EBREAKDOWN) {
            rc = GG_EBREAKDOWN;
            set_error(breakdown_msg(q, o[q]));             // (descending: the first such scenario's stays)
        } else if (o[q].r.status && rc == GG_OK) {
            rc = GG_NOT_CONVERGED;
        }
    }
    return rc;
}

void fill_outcome(Outcome &o, const BiState &h, float ms)
{
    int ret = GG_NOT_CONVERGED;
    if (h.done & (SR_CONV | SR_INIT)) ret = GG_OK;
    else if (h.done & SR_BREAKDOWN) ret = GG_EBREAKDOWN;
    o.r.status = ret;
    o.r.iters = h.it;
    o.r.inner_iters = h.it;
    o.r.restarts = 0;
    o.r.relres = h.resid;
    o.r.solve_ms = ms;
    o.why = h.why;
    o.bad = h.bad;
}

// A scenario that broke down may hold values that are not finite in its
// vectors, padding included, and NaN there would reach every dot of the next
// batch on this arena (the single solve: zero_vectors).  Its vectors and
// partials back to +0; the control block, history and granules stay.
void rezero(gg_solver *s, const BiBatchWs &a, int q)
{
    char *lo = reinterpret_cast<char *>(zq(a.x, a.arena.zs, q));
    const size_t bytes = (size_t)(reinterpret_cast<const char *>(a.bs) - reinterpret_cast<const char *>(a.x));
    GG_HIP(hipMemsetAsync(lo, 0, bytes, s->st));
}

int solve_bi_batch_once(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                        const gg_options *opt, gg_result *res)
{
    const int max_iter = opt->max_iter;
    ensure_bi_batch(s, S, (long long)max_iter + 1);
    BiBatchWs &a = *s->bi_batch;
    const Ctx c{s, &a, S, s->G, s->Ppad, a.arena.zs};
    hipStream_t st = s->st;
    stage_in(s, a.arena, d_b, ldb, d_x, ldx, a.b, a.x,
             [&] { launch_init_bi_state_b(a.bs, c.zs, S, opt->tol, max_iter, st); });
    a.ring.begin(s, a.arena, a.bs, "batched BiCGStab solve: wavefront boundary wait timed out");
    enqueue_start_b(c);

    // chunks of iterations, the host one chunk ahead (short_recurrence.h): chunk
    // c + 1 goes in before the control blocks after chunk c are read.  In a
    // transient the first chunk is the previous step's largest count + 2
    const int K = kBiBatchChunk;
    int next = 0;                                       // first iteration not yet enqueued
    auto enqueue = [&](int len) {
        const int k1 = (int)std::min<long long>((long long)next + len, max_iter);
        enqueue_iterations_b(c, next, k1);
        next = k1;
        a.ring.post();
    };
    enqueue(s->batch_iter_hint > 0 ? s->batch_iter_hint + 2 : K);
    enqueue(K);
    std::vector<BiState> hs(S);
    while (true) {
        const BiState *h = a.ring.wait_oldest();
        bool over = true;
        for (int q = 0; q < S; q++) over = over && (h[q].done || h[q].it >= max_iter);
        if (over) {
            std::copy(h, h + S, hs.begin());
            break;
        }
        enqueue(K);
    }
    const float ms = stage_out(s, a.arena, a.ring, a.x, d_x, ldx);
    std::vector<Outcome> out(S);
    a.seq = false;
    for (int q = 0; q < S; q++) {
        a.arena.hist_len[q] = (long long)hs[q].it + 1;
        fill_outcome(out[q], hs[q], ms);
        if (out[q].r.status == GG_EBREAKDOWN) rezero(s, a, q);
        if (res) res[q] = out[q].r;
    }
    return batch_status(S, out);
}

// scenario by scenario on the single BiCGStab solve (configurations the batched
// launches do not cover, GG_BATCH_SEQ=1); a scenario that breaks down stops,
// the others run
int solve_bi_batch_seq(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                       const gg_options *opt, gg_result *res)
{
    BiBatchWs *B = ws(s);
    B->seq = true;
    B->seq_hist.assign(S, {});
    gg_options o = *opt;
    o.flags = GG_SOLVE_BICGSTAB;
    std::vector<Outcome> out(S);
    for (int q = 0; q < S; q++) {
        const int e = solve_one(s, d_b + (long long)q * ldb, d_x + (long long)q * ldx, &o, &out[q].r);
        if (e < 0 && e != GG_EBREAKDOWN) return e;
        if (e == GG_EBREAKDOWN) {
            // the single solve's control block still holds the scalar
            BiState h{};
            GG_HIP(hipMemcpy(&h, s->bis.p, sizeof h, hipMemcpyDeviceToHost));
            out[q].why = h.why;
            out[q].bad = h.bad;
        }
        B->seq_hist[q] = s->last_hist;
        if (res) res[q] = out[q].r;
    }
    return batch_status(S, out);
}

}  // namespace

int solve_bicgstab_batch(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                         const gg_options *opt, gg_result *res)
{
    GG_REQUIRE(s->have_A, GG_ESTATE, "gg_solve_bicgstab_batch: no matrix (call gg_set_matrix)");
    GG_REQUIRE(s->pkind >= 0, GG_ESTATE, "gg_solve_bicgstab_batch: no preconditioner (call gg_set_precond_*)");
    GG_REQUIRE(opt, GG_EINVAL, "gg_solve_bicgstab_batch: null options");
    GG_REQUIRE(S >= 1, GG_EINVAL, "gg_solve_bicgstab_batch: nrhs must be >= 1");
    GG_REQUIRE(opt->restart >= 1 && opt->restart <= 512, GG_EINVAL,
               "gg_solve_bicgstab_batch: restart must be in [1, 512]");
    GG_REQUIRE(opt->max_iter >= 0, GG_EINVAL, "gg_solve_bicgstab_batch: negative max_iter");
    GG_REQUIRE((opt->flags & ~GG_SOLVE_BICGSTAB) == 0, GG_EINVAL,
               "gg_solve_bicgstab_batch: the only flag is GG_SOLVE_BICGSTAB (the entry point names the method)");
    GG_REQUIRE(s->pkind != GG_PRECOND_SPLIT && s->pkind != GG_PRECOND_USER && s->pkind != GG_PRECOND_USER_SPLIT,
               GG_EINVAL,
               "gg_solve_bicgstab_batch: BiCGStab takes a left preconditioner built by the library (NONE, DIAG, "
               "AINV, ILU0, ILUK, LU), not the split or caller-supplied ones");
    GG_REQUIRE(ldb >= s->A.n && ldx >= s->A.n, GG_EINVAL, "gg_solve_bicgstab_batch: leading dimension below n");
    GG_HIP(hipSetDevice(s->device));
    s->batch_last = BATCH_BICGSTAB;
    if (!batch_engine_on(s)) return solve_bi_batch_seq(s, S, d_b, ldb, d_x, ldx, opt, res);
    for (int attempt = 0;; attempt++) {
        try {
            return solve_bi_batch_once(s, S, d_b, ldb, d_x, ldx, opt, res);
        } catch (Fallback &f) {
            // IEEE division for the solver's life, repeat (d_x is written only at the end)
            GG_HIP(hipStreamSynchronize(s->st));
            if (attempt >= 2) throw Error{GG_EHIP, "gg_solve_bicgstab_batch: fallbacks exhausted"};
            apply_fallback(s, f);
        }
    }
}

long long bicgstab_batch_history(gg_solver *s, int q, double *out, long long cap)
{
    BiBatchWs *B = s->bi_batch;
    GG_REQUIRE(B, GG_ESTATE, "gg_batch_history: no batched solve holds that scenario");
    if (B->seq) {
        GG_REQUIRE(q >= 0 && q < (int)B->seq_hist.size() && !B->seq_hist[q].empty(), GG_ESTATE,
                   "gg_batch_history: no batched solve holds that scenario");
        const std::vector<double> &h = B->seq_hist[q];
        const long long n = (long long)h.size();
        if (out && cap > 0) std::copy(h.begin(), h.begin() + std::min(n, cap), out);
        return n;
    }
    return B->arena.history(B->hist, q, out, cap);
}

}  // namespace gg

// ======================================================================= C ABI
using namespace gg;

extern "C" {

int gg_solve_bicgstab_batch_device(gg_solver *s, int nrhs, const double *d_b, long long ldb, double *d_x,
                                   long long ldx, const gg_options *opt, gg_result *res)
{
    GG_API_BEGIN
    GG_REQUIRE(s && d_b && d_x, GG_EINVAL, "null argument");
    return solve_bicgstab_batch(s, nrhs, d_b, ldb, d_x, ldx, opt, res);
    GG_API_END
}

int gg_solve_bicgstab_batch(gg_solver *s, int nrhs, const double *b, long long ldb, double *x, long long ldx,
                            const gg_options *opt, gg_result *res)
{
    GG_API_BEGIN
    return solve_batch_host(s, solve_bicgstab_batch, "gg_solve_bicgstab_batch", false, nrhs, b, ldb, x, ldx, opt,
                            res);
    GG_API_END
}

int gg_transient_bicgstab_batch(gg_solver *s, int nrhs, int nsteps, double h, const double *cdiag,
                                const int *src_off, const int *src_node, const int *src_kind, const int *src_ptr,
                                const double *src_data, int nport, const int *port, double *x,
                                const gg_options *opt, double *port_out, int *iters_total)
{
    GG_API_BEGIN
    return transient_batch(s, BATCH_BICGSTAB, nrhs, nsteps, h, cdiag, src_off, src_node, src_kind, src_ptr, src_data,
                           nport, port, x, opt, port_out, iters_total);
    GG_API_END
}

}  // extern "C"
