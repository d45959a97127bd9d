// cg_batch.hip -- the many-RHS conjugate-gradient solve: nrhs independent
// right-hand sides on ONE matrix and preconditioner, every launch of a CG
// iteration serving all scenarios (DESIGN.md "CG batch").
//
// The method is cg.hip's, the batch is batch.hip's: scenario q keeps its own
// vectors, partials, control block (CgState) and history in an arena of its
// own, q * zs bytes after scenario 0's, and an iteration is seven launches for
// all scenarios together --
//   launch_spmv_b     q = A p         (A's entries read once per 8 scenarios)
//   launch_cg_pq      partials of p . q
//   launch_cg_xr      alpha; x = alpha p + x; r = (-alpha) q + r
//   launch_trsv_b L, U   z = M r      (one wavefront dependency chain for all)
//   launch_cg_rz      partials of r . z and z . z
//   launch_cg_p       res, beta; p = beta p + z
// Per scenario the arithmetic is the single solve's -- the same kernels with a
// scenario offset -- so scenario q's status, count, history and solution are
// bit-identical to gg_solve_device(GG_SOLVE_CG) on that right-hand side alone.
// A scenario whose gate is closed (converged, converged at the start, broken
// down, max_iter reached) drops out of every launch; the others go on.
//
// Iterations are enqueued in chunks with the host one chunk ahead of the
// control blocks it has read (batch_common.h's ReadRing, as the GMRES batch);
// there is no host synchronization per iteration.  The batch ends when a
// read-back shows every scenario over; the launches enqueued behind that point
// are gated off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "batch_common.h"

namespace gg {

// The work space: the arena and read-back ring (batch_common.h), scenario 0's
// arrays in the arena, and the histories of a scenario-by-scenario run.
struct CgBatchWs {
    BatchArena arena;                    // (no method key: 0)
    ReadRing<CgState> ring;
    CgState *cs = nullptr;
    double *x = nullptr, *b = nullptr, *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr, *bb = nullptr,
           *t1 = nullptr, *part = nullptr, *hist = nullptr;
    // the last solve's histories: arena.hist_len (batched), or the vectors
    // themselves (scenario by scenario)
    bool seq = false;
    std::vector<std::vector<double>> seq_hist;
};

void cg_batch_release(gg_solver *s)
{
    delete s->cg_batch;
    s->cg_batch = nullptr;
}

namespace {

// iterations per chunk after the first (GG_CG_BATCH_CHUNK).  A read-back round
// trip has to hide behind the chunk in flight, and a batch that is over leaves
// up to two chunks of launches that read their gates and return: seven
// dispatches per such iteration, which a transient step of ~11 iterations
// feels.  8 measured 6 % less time than the single solve's 32 on the C5
// transient (DESIGN.md "CG batch").  It changes no bits.
int cg_batch_chunk()
{
    static const int k = [] {
        const char *e = std::getenv("GG_CG_BATCH_CHUNK");
        const int v = e ? std::atoi(e) : 8;
        return v >= 1 ? v : 8;
    }();
    return k;
}

CgBatchWs *ws(gg_solver *s)
{
    if (!s->cg_batch) s->cg_batch = new CgBatchWs;
    return s->cg_batch;
}

void ensure_cg_batch(gg_solver *s, int S, long long hist_need)
{
    CgBatchWs *B = ws(s);
    BatchArena &A = B->arena;
    if (A.fits(s, S, hist_need, 0)) return;
    A.begin(s, S, hist_need, 0);
    const long long P = s->Ppad;
    A.take(B->x, P);
    A.take(B->b, P);
    A.take(B->r, P);
    A.take(B->z, P);
    A.take(B->p, P);
    A.take(B->q, P);
    A.take(B->bb, P);
    A.take(B->t1, P);
    A.take(B->part, 3 * 1024);           // p.q | r.z, z.z (cg.hip)
    A.take(B->cs, 1);
    A.take(B->hist, A.hist_cap);
    A.take(A.Lg, A.ngL);
    A.take(A.Ug, A.ngU);
    A.commit(s->st);
    B->ring.alloc(S);
}

struct Ctx {
    gg_solver *s;
    CgBatchWs *B;
    int S, G;
    long long P, zs;
};

// Cg::enqueue_start for every scenario
void enqueue_start_b(const Ctx &c)
{
    gg_solver *s = c.s;
    const CgBatchWs &a = *c.B;
    const Gate none;
    batch_minv(s, a.arena, none, a.b, a.t1, a.bb);                                  // bb = M b
    launch_dot(none, a.bb, a.bb, a.part, c.G, c.P, s->st, Batch{c.S, c.zs});
    launch_normb(a.part, c.G, &a.cs->normb, s->st, Batch{c.S, c.zs});
    launch_spmv_b(none, s->dA, a.x, a.b, a.r, true, c.S, c.zs, s->st);              // r = b - A x
    batch_minv(s, a.arena, none, a.r, a.t1, a.z);                                   // z = M r
    launch_cg_rz(none, a.r, a.z, a.part + 1024, c.G, c.P, s->st, Batch{c.S, c.zs});
    launch_cg_p(none, 0, true, a.cs, a.part + 1024, c.G, a.p, a.z, a.hist, c.P, s->st, Batch{c.S, c.zs});   // p = z
}

// Cg::enqueue_iterations for every scenario, each launch gated per scenario
void enqueue_iterations_b(const Ctx &c, int k0, int k1)
{
    gg_solver *s = c.s;
    const CgBatchWs &a = *c.B;
    for (int k = k0; k < k1; k++) {
        Gate g;
        g.done = &a.cs->done;
        g.mask = ~0;
        g.nit = &a.cs->max_iter;
        g.i = k;
        launch_spmv_b(g, s->dA, a.p, nullptr, a.q, false, c.S, c.zs, s->st);        // q = A p
        launch_cg_pq(g, a.p, a.q, a.part, c.G, c.P, s->st, Batch{c.S, c.zs});
        launch_cg_xr(g, k, a.cs, a.part, c.G, a.x, a.p, a.r, a.q, c.P, s->st, Batch{c.S, c.zs});
        batch_minv(s, a.arena, g, a.r, a.t1, a.z);                                  // z = M r
        launch_cg_rz(g, a.r, a.z, a.part + 1024, c.G, c.P, s->st, Batch{c.S, c.zs});
        launch_cg_p(g, k, false, a.cs, a.part + 1024, c.G, a.p, a.z, a.hist, c.P, s->st, Batch{c.S, c.zs});
    }
}

std::string breakdown_msg(int q, int it)
{
    return "gg_solve_cg_batch: conjugate gradients broke down in scenario " + std::to_string(q) + " at iteration " +
           std::to_string(it) + " (p.Ap or r.Mr not positive: A and M must be symmetric positive definite)";
}

// what a batch returns from its scenarios' statuses
int batch_status(int S, const std::vector<gg_result> &r)
{
    int rc = GG_OK;
    for (int q = S - 1; q >= 0; q--) {
        if (r[q].status == GG_EBREAKDOWN) {
            rc = GG_EBREAKDOWN;
            set_error(breakdown_msg(q, r[q].iters));       // (descending: the first such scenario's stays)
        } else if (r[q].status && rc == GG_OK) {
            rc = GG_NOT_CONVERGED;
        }
    }
    return rc;
}

int solve_cg_batch_once(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                        const gg_options *opt, gg_result *res)
{
    const int max_iter = opt->max_iter;
    ensure_cg_batch(s, S, (long long)max_iter + 1);
    CgBatchWs &a = *s->cg_batch;
    const Ctx c{s, &a, S, s->G, s->Ppad, a.arena.zs};
    hipStream_t st = s->st;
    stage_in(s, a.arena, d_b, ldb, d_x, ldx, a.b, a.x,
             [&] { launch_init_cg_state_b(a.cs, c.zs, S, opt->tol, max_iter, st); });
    a.ring.begin(s, a.arena, a.cs, "batched CG solve: wavefront boundary wait timed out");
    enqueue_start_b(c);

    // chunks of iterations, the host one chunk ahead (short_recurrence.h): chunk
    // c + 1 goes in before the control blocks after chunk c are read.  In a
    // transient the first chunk is the previous step's largest count + 2
    const int K = cg_batch_chunk();
    int next = 0;                                       // first iteration not yet enqueued
    auto enqueue = [&](int len) {
        const int k1 = (int)std::min<long long>((long long)next + len, max_iter);
        enqueue_iterations_b(c, next, k1);
        next = k1;
        a.ring.post();
    };
    enqueue(s->batch_iter_hint > 0 ? s->batch_iter_hint + 2 : K);
    enqueue(K);
    std::vector<CgState> hs(S);
    while (true) {
        const CgState *h = a.ring.wait_oldest();
        bool over = true;
        for (int q = 0; q < S; q++) over = over && (h[q].done || h[q].it >= max_iter);
        if (over) {
            std::copy(h, h + S, hs.begin());
            break;
        }
        enqueue(K);
    }
    const float ms = stage_out(s, a.arena, a.ring, a.x, d_x, ldx);
    std::vector<gg_result> out(S);
    a.seq = false;
    for (int q = 0; q < S; q++) {
        const CgState &h = hs[q];
        a.arena.hist_len[q] = (long long)h.it + 1;
        int ret = GG_NOT_CONVERGED;
        if (h.done & (SR_CONV | SR_INIT)) ret = GG_OK;
        else if (h.done & SR_BREAKDOWN) ret = GG_EBREAKDOWN;
        out[q].status = ret;
        out[q].iters = h.it;
        out[q].inner_iters = h.it;
        out[q].restarts = 0;
        out[q].relres = h.resid;
        out[q].solve_ms = ms;
        if (res) res[q] = out[q];
    }
    return batch_status(S, out);
}

// scenario by scenario on the single CG solve (configurations the batched
// launches do not cover, GG_BATCH_SEQ=1); a scenario that breaks down stops,
// the others run
int solve_cg_batch_seq(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                       const gg_options *opt, gg_result *res)
{
    CgBatchWs *B = ws(s);
    B->seq = true;
    B->seq_hist.assign(S, {});
    gg_options o = *opt;
    o.flags = GG_SOLVE_CG;
    std::vector<gg_result> out(S);
    for (int q = 0; q < S; q++) {
        const int e = solve_one(s, d_b + (long long)q * ldb, d_x + (long long)q * ldx, &o, &out[q]);
        if (e < 0 && e != GG_EBREAKDOWN) return e;
        B->seq_hist[q] = s->last_hist;
        if (res) res[q] = out[q];
    }
    return batch_status(S, out);
}

}  // namespace

int solve_cg_batch(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                   const gg_options *opt, gg_result *res)
{
    GG_REQUIRE(s->have_A, GG_ESTATE, "gg_solve_cg_batch: no matrix (call gg_set_matrix)");
    GG_REQUIRE(s->pkind >= 0, GG_ESTATE, "gg_solve_cg_batch: no preconditioner (call gg_set_precond_*)");
    GG_REQUIRE(opt, GG_EINVAL, "gg_solve_cg_batch: null options");
    GG_REQUIRE(S >= 1, GG_EINVAL, "gg_solve_cg_batch: nrhs must be >= 1");
    GG_REQUIRE(opt->restart >= 1 && opt->restart <= 512, GG_EINVAL, "gg_solve_cg_batch: restart must be in [1, 512]");
    GG_REQUIRE(opt->max_iter >= 0, GG_EINVAL, "gg_solve_cg_batch: negative max_iter");
    GG_REQUIRE((opt->flags & ~GG_SOLVE_CG) == 0, GG_EINVAL,
               "gg_solve_cg_batch: the only flag is GG_SOLVE_CG (the entry point names the method)");
    GG_REQUIRE(s->pkind != GG_PRECOND_SPLIT && s->pkind != GG_PRECOND_USER && s->pkind != GG_PRECOND_USER_SPLIT,
               GG_EINVAL,
               "gg_solve_cg_batch: conjugate gradients take a left preconditioner built by the library (NONE, "
               "DIAG, AINV, ILU0, ILUK, LU), not the split or caller-supplied ones");
    GG_REQUIRE(ldb >= s->A.n && ldx >= s->A.n, GG_EINVAL, "gg_solve_cg_batch: leading dimension below n");
    GG_HIP(hipSetDevice(s->device));
    s->batch_last = BATCH_CG;
    if (!batch_engine_on(s)) return solve_cg_batch_seq(s, S, d_b, ldb, d_x, ldx, opt, res);
    for (int attempt = 0;; attempt++) {
        try {
            return solve_cg_batch_once(s, S, d_b, ldb, d_x, ldx, opt, res);
        } catch (Fallback &f) {
            // IEEE division for the solver's life, repeat (d_x is written only at the end)
            GG_HIP(hipStreamSynchronize(s->st));
            if (attempt >= 2) throw Error{GG_EHIP, "gg_solve_cg_batch: fallbacks exhausted"};
            apply_fallback(s, f);
        }
    }
}

long long cg_batch_history(gg_solver *s, int q, double *out, long long cap)
{
    CgBatchWs *B = s->cg_batch;
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

int gg_solve_cg_batch_device(gg_solver *s, int nrhs, const double *d_b, long long ldb, double *d_x, long long ldx,
                             const gg_options *opt, gg_result *res)
{
    GG_API_BEGIN
    GG_REQUIRE(s && d_b && d_x, GG_EINVAL, "null argument");
    return solve_cg_batch(s, nrhs, d_b, ldb, d_x, ldx, opt, res);
    GG_API_END
}

int gg_solve_cg_batch(gg_solver *s, int nrhs, const double *b, long long ldb, double *x, long long ldx,
                      const gg_options *opt, gg_result *res)
{
    GG_API_BEGIN
    return solve_batch_host(s, solve_cg_batch, "gg_solve_cg_batch", false, nrhs, b, ldb, x, ldx, opt, res);
    GG_API_END
}

int gg_transient_cg_batch(gg_solver *s, int nrhs, int nsteps, double h, const double *cdiag, const int *src_off,
                          const int *src_node, const int *src_kind, const int *src_ptr, const double *src_data,
                          int nport, const int *port, double *x, const gg_options *opt, double *port_out,
                          int *iters_total)
{
    GG_API_BEGIN
    return transient_batch(s, BATCH_CG, nrhs, nsteps, h, cdiag, src_off, src_node, src_kind, src_ptr, src_data, nport,
                           port, x, opt, port_out, iters_total);
    GG_API_END
}

}  // extern "C"
