// batch.hip -- the many-RHS solve: nrhs independent right-hand sides on ONE
// matrix and preconditioner, carried through one set of launches.
//
// "many-RHS" = independent source scenarios solved as a
// batch.  The reference runs its step driver once per scenario
// (src/mna_solve_gpu_gmres.cpp:564-647 around GMRES_GPU_tran,
// src/gmres.cu:2736-2827).  Here scenario q keeps its own Krylov basis, H,
// Givens rotations, residual history and control block -- one arena per
// scenario, q * zs bytes after scenario 0's -- and every launch of a GMRES
// phase serves all scenarios at once:
//   * the SpMV reads A's sliced-ELL entries once for up to 8 scenarios
//     (k_spmv_sell_b);
//   * the 2D wavefront triangular solves run every scenario's bands side by
//     side in one launch (k_trsv_wave2d_batch): one dependency chain of
//     nx + ny - 1 steps for all of them instead of one per scenario;
//   * the MGS kernels (k_dot, k_mgs_step, k_arnoldi_finalize) reduce nrhs
//     dot products per launch, the update and the scalar kernels likewise.
// Per scenario the arithmetic is the single-RHS solve's -- the same kernels
// with a scenario offset -- so scenario q's history, iteration count and
// solution are bit-identical to gg_solve_device on that right-hand side alone
// (whose persistent and per-step orthogonalizations are bit-identical too).
// A scenario whose gate is closed (converged, restart-converged, max_iter
// exhausted) drops out of every launch; the others go on.
//
// The restart cycle is enqueued in chunks of inner iterations (GG_BATCH_CHUNK,
// default 3) with the host one chunk ahead, instead of m gated iterations: a
// transient step converges in ~9 of m = 32 iterations, and a gated launch
// still costs its dispatch.  When every scenario's cycle is over at a chunk's
// read-back, the cycle's tail (Update, residual, its norm) is enqueued; the
// host waits for the tail's control blocks only when some scenario did not
// converge inside the cycle (restart or max_iter).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "batch_common.h"

namespace gg {

namespace {

// GG_BATCH_MGS: the orthogonalization of a batched inner iteration -- 0 the
// per-step kernels with every scenario in each launch (k_dot, k_mgs_step,
// k_arnoldi_finalize: i + 3 launches), 1 the single-scenario persistent kernel
// once per scenario (k_arnoldi_persist: w and the basis step in registers, the
// same reduction tree, so the same bits)
int batch_mgs()
{
    static const int k = [] {
        const char *e = std::getenv("GG_BATCH_MGS");
        return e ? std::atoi(e) : 1;
    }();
    return k;
}

// GG_BATCH_MGS2=0: one persistent launch per scenario instead of per pair
bool batch_mgs2()
{
    static const bool on = [] {
        const char *e = std::getenv("GG_BATCH_MGS2");
        return !(e && e[0] == '0');
    }();
    return on;
}

int batch_chunk()
{
    static const int k = [] {
        const char *e = std::getenv("GG_BATCH_CHUNK");
        const int v = e ? std::atoi(e) : 3;
        return v >= 1 ? v : 3;
    }();
    return k;
}

}  // namespace

// The work space: the arena and read-back ring (batch_common.h), scenario 0's
// arrays in the arena, and the orthogonalization's state.
struct BatchWs {
    BatchArena arena;                    // its method key: the restart length m
    ReadRing<DevState> ring;
    DevState *ds = nullptr;
    double *V = nullptr, *w = nullptr, *ww = nullptr, *r = nullptr, *rr = nullptr, *bb = nullptr, *t1 = nullptr,
           *xv = nullptr, *bv = nullptr, *pA = nullptr, *pB = nullptr, *H = nullptr, *sv = nullptr, *cs = nullptr,
           *sn = nullptr, *y = nullptr, *hist = nullptr;
    // the persistent orthogonalization (GG_BATCH_MGS 1): its all-gather granules
    // per scenario (m (m+2) G, then m (m+2) sums) and XCD slots, and the
    // solver-wide election words; persist = admitted (co-residency), cleared
    // for the solver's life when a launch was not co-resident
    bool persist = false;
    bool persist2 = false;               // two scenarios per persistent launch (k_arnoldi_persist2)
    long long ngran = 0, nxgran = 0;
    unsigned long long *gran = nullptr, *xgran = nullptr;
    DBuf<unsigned long long> elect;
    unsigned long long seq = 0;
    // the orthogonalization the last batched solve ran to its end with
    // (gg_batch_mgs_kernel): 2 k_arnoldi_persist2 (an odd last scenario on
    // k_arnoldi_persist), 1 k_arnoldi_persist per scenario, 0 the per-step kernels
    int ran_mgs = -1;
};

void batch_release(gg_solver *s)
{
    delete s->batch;
    s->batch = nullptr;
    cg_batch_release(s);
    bicgstab_batch_release(s);
}

namespace {

// one scenario's outcome (the single solve's bookkeeping, solver.hip
// solve_device_once)
struct Track {
    bool fin = false, cyc_over = false;
    int ret = 1, iters = 0, inner = 0, restarts = 0, prev_j = 1;
    long long hist_len = 1;
    double relres = 0.0;
};

bool batchable(const gg_solver *s)
{
    const bool left = s->pkind == GG_PRECOND_ILU0 || s->pkind == GG_PRECOND_ILUK || s->pkind == GG_PRECOND_LU;
    if (!left || !s->wave) return false;
    if (s->L.kind != DevTri::WAVE2D || s->U.kind != DevTri::WAVE2D) return false;
    const char *e = std::getenv("GG_BATCH_SEQ");          // A/B, tests: scenario by scenario
    if (e && e[0] == '1') return false;
    DevTri &L = const_cast<DevTri &>(s->L), &U = const_cast<DevTri &>(s->U);
    L.fast = s->div_mode;
    U.fast = s->div_mode;
    return trsv_batchable(L) && trsv_batchable(U);
}

void ensure_batch(gg_solver *s, int S, int m, long long hist_need)
{
    if (s->batch && s->batch->arena.fits(s, S, hist_need, m)) return;
    batch_release(s);
    BatchWs *B = new BatchWs;
    s->batch = B;
    BatchArena &A = B->arena;
    A.begin(s, S, hist_need, m);
    const long long P = s->Ppad;
    A.take(B->V, (long long)(m + 1) * P);
    A.take(B->w, P);
    A.take(B->ww, P);
    A.take(B->r, P);
    A.take(B->rr, P);
    A.take(B->bb, P);
    A.take(B->t1, P);
    A.take(B->xv, P);
    A.take(B->bv, P);
    A.take(B->pA, 1024);
    A.take(B->pB, 1024);
    A.take(B->H, (long long)(m + 1) * m);
    A.take(B->sv, m + 1);
    A.take(B->cs, m + 1);
    A.take(B->sn, m + 1);
    A.take(B->y, m + 1);
    A.take(B->hist, A.hist_cap);
    A.take(B->ds, 1);
    A.take(A.Lg, A.ngL);
    A.take(A.Ug, A.ngU);
    {
        const int pj = arnoldi_persist_units(s->G, s->Ppad);
        const int xr = pj ? arnoldi_persist_extra(pj) : 0;
        B->persist = batch_mgs() == 1 && pj != 0 && s->G + xr <= arnoldi_persist_max_blocks(pj);
        B->persist2 = B->persist && S > 1 && xr == 0 && mgs_gather_form() == 2 && mgs_prefetch() == 1 &&
                      arnoldi_persist2_units(s->G, s->Ppad) != 0 && batch_mgs2();
        if (B->persist) {
            B->ngran = (long long)m * (m + 2) * (s->G + 1);
            B->nxgran = (long long)m * (m + 2) * kMgsXcdWords;
            A.take(B->gran, B->ngran);
            A.take(B->xgran, B->nxgran);
            B->elect.alloc(kMgsElectWords);
            GG_HIP(hipMemsetAsync(B->elect.p, 0, kMgsElectWords * sizeof(unsigned long long), s->st));
        }
    }
    A.commit(s->st);
    B->ring.alloc(S);
}

struct BatchAbort {};     // a persistent orthogonalization grid was not co-resident

struct Ctx {
    gg_solver *s;
    BatchWs *B;
    int S, m, G;
    long long P, zs;
    UnitMap um;
};

void enqueue_init_b(const Ctx &c)
{
    gg_solver *s = c.s;
    const BatchWs &a = *c.B;
    Gate none;
    batch_minv(s, a.arena, none, a.bv, a.t1, a.bb);                                 // bb = M b
    launch_dot(none, a.bb, a.bb, a.pA, c.G, c.P, s->st, Batch{c.S, c.zs});
    launch_set_normb(a.pA, c.G, a.ds, s->st, Batch{c.S, c.zs});
    launch_spmv_b(none, s->dA, a.xv, a.bv, a.rr, true, c.S, c.zs, s->st);        // rr = b - A x
    batch_minv(s, a.arena, none, a.rr, a.t1, a.r);                                  // r = M rr
    launch_dot(none, a.r, a.r, a.pA, c.G, c.P, s->st, Batch{c.S, c.zs});
    launch_init_beta(a.pA, c.G, a.ds, a.hist, s->st, Batch{c.S, c.zs});
}

// inner iterations [i0, i1) of the cycle (src/gmres.cu:566-717's loop body:
// w = M^-1 A v_i, MGS, Givens, residual check), every one gated per scenario
void enqueue_iters_b(const Ctx &c, int i0, int i1)
{
    gg_solver *s = c.s;
    const BatchWs &a = *c.B;
    for (int i = i0; i < i1; i++) {
        Gate gi;
        gi.done = &a.ds->done;
        gi.mask = ~0;
        gi.nit = &a.ds->nit;
        gi.i = i;
        const double *vi = a.V + (long long)i * c.P;
        launch_spmv_b(gi, s->dA, vi, nullptr, a.ww, false, c.S, c.zs, s->st);   // ww = A v_i
        batch_minv(s, a.arena, gi, a.ww, a.t1, a.w);                                // w = M^-1 ww
        if (c.B->persist) {
            // the persistent kernel: two scenarios per launch (k_arnoldi_persist2),
            // or one (k_arnoldi_persist) -- the same tree, the same bits
            for (int q = 0; q < c.S; q++) {
                Gate gq = gi;
                gq.done = zq(gi.done, c.zs, q);
                gq.nit = zq(gi.nit, c.zs, q);
                unsigned long long *gr = zq(a.gran, c.zs, q);
                if (c.B->persist2 && q + 1 < c.S) {
                    launch_arnoldi_persist2(gq, c.zs, i, c.m, zq(a.ds, c.zs, q), zq(a.w, c.zs, q), zq(a.V, c.zs, q), c.P,
                                            zq(a.H, c.zs, q), zq(a.cs, c.zs, q), zq(a.sn, c.zs, q),
                                            zq(a.sv, c.zs, q), zq(a.hist, c.zs, q),
                                            gr + (size_t)i * (c.m + 2) * c.G, c.G, c.P, s->err.p,
                                            zq(a.xgran, c.zs, q) + (size_t)i * (c.m + 2) * kMgsXcdWords,
                                            c.B->elect.p, ++c.B->seq, c.um, s->st);
                    q++;
                    continue;
                }
                launch_arnoldi_persist(gq, i, c.m, zq(a.ds, c.zs, q), zq(a.w, c.zs, q), zq(a.V, c.zs, q), c.P,
                                       zq(a.H, c.zs, q), zq(a.cs, c.zs, q), zq(a.sn, c.zs, q), zq(a.sv, c.zs, q),
                                       zq(a.hist, c.zs, q), gr + (size_t)i * (c.m + 2) * c.G,
                                       gr + (size_t)c.m * (c.m + 2) * c.G + (size_t)i * (c.m + 2), c.G, c.P,
                                       s->err.p, zq(a.xgran, c.zs, q) + (size_t)i * (c.m + 2) * kMgsXcdWords,
                                       c.B->elect.p, ++c.B->seq, c.um, s->st);
            }
            continue;
        }
        double *pin = a.pA, *pout = a.pB;
        launch_dot(gi, a.w, a.V, pin, c.G, c.P, s->st, Batch{c.S, c.zs});   // <w, v_0>
        for (int k = 0; k <= i; k++) {
            const double *vk = a.V + (long long)k * c.P;
            const double *vn = (k < i) ? a.V + (long long)(k + 1) * c.P : a.w;
            launch_mgs_step(gi, i, k, c.m, a.w, vk, vn, pin, pout, a.H, c.G, c.P, s->st, Batch{c.S, c.zs});
            std::swap(pin, pout);
        }
        launch_arnoldi_finalize(gi, i, c.m, a.ds, pin, c.G, a.w, a.V + (long long)(i + 1) * c.P, a.H, a.cs, a.sn,
                                a.sv, a.hist, c.P, s->st, Batch{c.S, c.zs});
    }
}

// the cycle's tail: x += V y, r = M (b - A x), beta, history, j += nit
void enqueue_tail_b(const Ctx &c)
{
    gg_solver *s = c.s;
    const BatchWs &a = *c.B;
    Gate gu;
    gu.done = &a.ds->done;
    gu.mask = DONE_RESTART | DONE_INIT | DONE_ABORT | DONE_FINAL | DONE_EXH;
    launch_update(gu, c.m, a.ds, a.H, a.sv, a.y, a.V, c.P, a.xv, c.G, c.P, s->st, c.um, Batch{c.S, c.zs});
    Gate gr;
    gr.done = &a.ds->done;
    gr.mask = ~0;
    launch_spmv_b(gr, s->dA, a.xv, a.bv, a.rr, true, c.S, c.zs, s->st);
    batch_minv(s, a.arena, gr, a.rr, a.t1, a.r);
    launch_dot(gr, a.r, a.r, a.pA, c.G, c.P, s->st, Batch{c.S, c.zs});
    launch_end_cycle(a.pA, c.G, a.ds, a.hist, s->st, Batch{c.S, c.zs});
}

int solve_batch_once(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                     const gg_options *opt, gg_result *res)
{
    const int m = opt->restart;
    const long long need = (long long)opt->max_iter + opt->max_iter / m + 4;
    ensure_batch(s, S, m, need);
    BatchWs &a = *s->batch;
    a.ran_mgs = -1;
    const Ctx c{s, &a, S, m, s->G, s->Ppad, a.arena.zs, solver_unit_map(s)};
    hipStream_t st = s->st;
    stage_in(s, a.arena, d_b, ldb, d_x, ldx, a.bv, a.xv,
             [&] { launch_init_state_b(a.ds, c.zs, S, opt->tol, opt->max_iter, m, st); });
    a.ring.begin(s, a.arena, a.ds, "batched solve: wavefront boundary wait timed out");
    enqueue_init_b(c);

    std::vector<Track> tr(S);
    const int K = batch_chunk();
    if (opt->max_iter < 1) {
        // no cycle: converged at the start or max_iter exhausted (j = 1 > max_iter)
        const DevState *h = a.ring.post_and_wait();
        for (int q = 0; q < S; q++) {
            tr[q].fin = true;
            tr[q].relres = h[q].resid;
            tr[q].ret = (h[q].done & DONE_INIT) ? 0 : 1;
            tr[q].iters = (h[q].done & DONE_INIT) ? 0 : opt->max_iter;
        }
    }
    int left = 0;
    for (const Track &t : tr) left += !t.fin;
    while (left > 0) {
        // ---- one restart cycle, in chunks of K inner iterations
        launch_init_cycle(a.ds, a.r, a.V, a.sv, c.G, c.P, st, Batch{S, c.zs});
        if (a.persist) {
            launch_fill_u64(a.gran, a.ngran, kSentinel, st, Batch{S, c.zs});
            launch_fill_u64(a.xgran, a.nxgran, kSentinel, st, Batch{S, c.zs});
        }
        for (Track &t : tr) t.cyc_over = t.fin;
        int issued = 0;
        auto chunk = [&]() {
            const int i1 = std::min(issued + K, m);
            enqueue_iters_b(c, issued, i1);
            issued = i1;
            a.ring.post(issued);                            // tagged with the iterations enqueued
        };
        chunk();
        if (issued < m) chunk();
        const DevState *h = nullptr;
        while (true) {
            int iend = 0;
            h = a.ring.wait_oldest(&iend);
            for (int q = 0; q < S; q++)
                if (h[q].done & DONE_ABORT) throw BatchAbort{};
            bool over = true;
            for (int q = 0; q < S; q++) {
                Track &t = tr[q];
                if (t.cyc_over) continue;
                const int d = h[q].done;
                if ((d & (DONE_INIT | DONE_EXH | DONE_INNER | DONE_RESTART)) || iend >= h[q].nit) t.cyc_over = true;
                else over = false;
            }
            if (over) break;
            if (issued < m) chunk();
            GG_REQUIRE(a.ring.pending(), GG_EHIP, "batched solve: cycle did not end after m iterations");
        }
        // the scenarios' outcomes as far as the last read-back decides them
        std::vector<DevState> hs(h, h + S);
        enqueue_tail_b(c);
        bool need_tail = false;
        for (int q = 0; q < S; q++) {
            Track &t = tr[q];
            if (t.fin) continue;
            const DevState &hq = hs[q];
            if (hq.done & DONE_INIT) {                      // converged at the start
                t.fin = true;
                t.ret = 0;
                t.iters = 0;
                t.hist_len = 1;
                t.relres = hq.resid;
            } else if (hq.done & DONE_INNER) {              // converged inside the cycle
                t.fin = true;
                t.ret = 0;
                t.restarts++;
                t.iters = t.prev_j + hq.conv_i;
                t.inner += hq.conv_i + 1;
                t.hist_len = hq.hist_len + hq.conv_i + 1;
                t.relres = hq.resid;
            } else {
                need_tail = true;
            }
        }
        if (need_tail) {
            const DevState *ht = a.ring.post_and_wait();
            for (int q = 0; q < S; q++) {
                Track &t = tr[q];
                if (t.fin) continue;
                const DevState &hq = ht[q];
                t.restarts++;
                t.inner += hq.nit;
                t.hist_len = hq.hist_len;
                t.relres = hq.resid;
                if (hq.done & DONE_RESTART) {
                    t.fin = true;
                    t.ret = 0;
                    t.iters = hq.j;
                } else if (hq.j > opt->max_iter) {          // while (j <= *max_iter) exhausted
                    t.fin = true;
                    t.ret = 1;
                    t.iters = opt->max_iter;                // the reference leaves *max_iter untouched
                } else {
                    t.prev_j = hq.j;
                }
            }
        }
        left = 0;
        for (const Track &t : tr) left += !t.fin;
    }
    const float ms = stage_out(s, a.arena, a.ring, a.xv, d_x, ldx);
    int rc = GG_OK;
    a.ran_mgs = a.persist2 ? 2 : a.persist ? 1 : 0;
    for (int q = 0; q < S; q++) {
        const Track &t = tr[q];
        a.arena.hist_len[q] = t.hist_len;
        if (t.ret) rc = 1;
        if (res) {
            res[q].status = t.ret;
            res[q].iters = t.iters;
            res[q].inner_iters = t.inner;
            res[q].restarts = t.restarts;
            res[q].relres = t.relres;
            res[q].solve_ms = ms;
        }
    }
    return rc;
}

// the solver object's own scenario-by-scenario engine (non-batchable
// configurations, GG_BATCH_SEQ=1)
int solve_batch_seq(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                    const gg_options *opt, gg_result *res)
{
    int rc = GG_OK;
    if (s->batch) s->batch->arena.hist_len.assign(S, 0);
    if (s->batch) s->batch->ran_mgs = -1;
    for (int q = 0; q < S; q++) {
        gg_result r{};
        const int e = solve_one(s, d_b + (long long)q * ldb, d_x + (long long)q * ldx, opt, &r);
        if (e < 0) return e;
        if (e) rc = e;
        if (res) res[q] = r;
    }
    return rc;
}

}  // namespace

// the engine behind gg_solve_batch_device (also the transient batch's step)
int solve_batch(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                const gg_options *opt, gg_result *res)
{
    GG_REQUIRE(s->have_A, GG_ESTATE, "gg_solve_batch: no matrix (call gg_set_matrix)");
    GG_REQUIRE(s->pkind >= 0, GG_ESTATE, "gg_solve_batch: no preconditioner (call gg_set_precond_*)");
    GG_REQUIRE(opt, GG_EINVAL, "gg_solve_batch: null options");
    GG_REQUIRE(S >= 1, GG_EINVAL, "gg_solve_batch: nrhs must be >= 1");
    GG_REQUIRE(opt->restart >= 1 && opt->restart <= 512, GG_EINVAL, "gg_solve_batch: restart must be in [1, 512]");
    GG_REQUIRE(opt->max_iter >= 0, GG_EINVAL, "gg_solve_batch: negative max_iter");
    GG_REQUIRE(opt->flags == 0, GG_EINVAL, "gg_solve_batch: no flags are defined for the batch");
    GG_REQUIRE(ldb >= s->A.n && ldx >= s->A.n, GG_EINVAL, "gg_solve_batch: leading dimension below n");
    GG_HIP(hipSetDevice(s->device));
    s->batch_last = BATCH_GMRES;
    if (!batchable(s)) return solve_batch_seq(s, S, d_b, ldb, d_x, ldx, opt, res);
    for (int attempt = 0;; attempt++) {
        try {
            return solve_batch_once(s, S, d_b, ldb, d_x, ldx, opt, res);
        } catch (BatchAbort &) {
            // not co-resident: the per-step kernels for the solver's life, repeat
            GG_HIP(hipStreamSynchronize(s->st));
            if (attempt >= 2) throw Error{GG_EHIP, "gg_solve_batch: fallbacks exhausted"};
            s->batch->persist = false;
            s->batch->persist2 = false;
        } catch (Fallback &f) {
            // a WD_RCP range miss: IEEE division for the solver's life, repeat
            // (d_x is written only at the end)
            GG_HIP(hipStreamSynchronize(s->st));
            if (attempt >= 2) throw Error{GG_EHIP, "gg_solve_batch: fallbacks exhausted"};
            apply_fallback(s, f);
        }
    }
}

bool batch_engine_on(gg_solver *s) { return batchable(s); }

std::string batch_mgs_kernel(gg_solver *s)
{
    const BatchWs *B = s->batch;
    if (s->batch_last != BATCH_GMRES || !B || B->ran_mgs <= 0) return "";
    const int J = arnoldi_persist_units(s->G, s->Ppad);
    if (B->ran_mgs == 2) return "k_arnoldi_persist2<" + std::to_string(J) + ">";
    return arnoldi_persist_name(J);
}

long long batch_history(gg_solver *s, int q, double *out, long long cap)
{
    if (s->batch_last == BATCH_CG) return cg_batch_history(s, q, out, cap);
    if (s->batch_last == BATCH_BICGSTAB) return bicgstab_batch_history(s, q, out, cap);
    GG_REQUIRE(s->batch, GG_ESTATE, "gg_batch_history: no batched solve holds that scenario");
    return s->batch->arena.history(s->batch->hist, q, out, cap);
}

}  // namespace gg

// ======================================================================= C ABI
using namespace gg;

extern "C" {

int gg_solve_batch_device(gg_solver *s, int nrhs, const double *d_b, long long ldb, double *d_x, long long ldx,
                          const gg_options *opt, gg_result *res)
{
    GG_API_BEGIN
    GG_REQUIRE(s && d_b && d_x, GG_EINVAL, "null argument");
    return solve_batch(s, nrhs, d_b, ldb, d_x, ldx, opt, res);
    GG_API_END
}

int gg_solve_batch(gg_solver *s, int nrhs, const double *b, long long ldb, double *x, long long ldx,
                   const gg_options *opt, gg_result *res)
{
    GG_API_BEGIN
    return solve_batch_host(s, solve_batch, "gg_solve_batch", true, nrhs, b, ldb, x, ldx, opt, res);
    GG_API_END
}

long long gg_batch_history(gg_solver *s, int rhs, double *out, long long cap)
{
    GG_API_BEGIN
    GG_REQUIRE(s, GG_EINVAL, "null solver");
    return batch_history(s, rhs, out, cap);
    GG_API_END
}

int gg_batch_engine(gg_solver *s)
{
    GG_API_BEGIN
    GG_REQUIRE(s, GG_EINVAL, "null solver");
    GG_REQUIRE(s->pkind >= 0, GG_ESTATE, "gg_batch_engine: no preconditioner");
    return batch_engine_on(s) ? 1 : 0;
    GG_API_END
}

int gg_batch_mgs_kernel(gg_solver *s, char *name, int cap)
{
    GG_API_BEGIN
    GG_REQUIRE(s && name && cap > 0, GG_EINVAL, "null argument");
    const std::string k = batch_mgs_kernel(s);
    std::snprintf(name, (size_t)cap, "%s", k.c_str());
    return (int)k.size();
    GG_API_END
}

int gg_transient_batch(gg_solver *s, int nrhs, int nsteps, double h, const double *cdiag, const int *src_off,
                       const int *src_node, const int *src_kind, const int *src_ptr, const double *src_data,
                       int nport, const int *port, double *x, const gg_options *opt, double *port_out,
                       int *iters_total)
{
    GG_API_BEGIN
    return transient_batch(s, BATCH_GMRES, nrhs, nsteps, h, cdiag, src_off, src_node, src_kind, src_ptr, src_data,
                           nport, port, x, opt, port_out, iters_total);
    GG_API_END
}

}  // extern "C"

// the transient loop of every scenario (gg_transient_batch; method BATCH_CG:
// gg_transient_cg_batch, BATCH_BICGSTAB: gg_transient_bicgstab_batch -- the step
// solved by solve_cg_batch / solve_bicgstab_batch with its first chunk sized by
// the previous step)
int gg::transient_batch(gg_solver *s, BatchMethod method, int nrhs, int nsteps, double h, const double *cdiag,
                        const int *src_off, const int *src_node, const int *src_kind, const int *src_ptr,
                        const double *src_data, int nport, const int *port, double *x, const gg_options *opt,
                        double *port_out, int *iters_total)
{
    GG_REQUIRE(s && opt && x && cdiag && src_off && iters_total, GG_EINVAL, "null argument");
    GG_REQUIRE(s->have_A, GG_ESTATE, "gg_transient_batch: no matrix");
    GG_REQUIRE(nrhs >= 1 && nsteps >= 0 && nport >= 0, GG_EINVAL, "gg_transient_batch: bad count");
    GG_REQUIRE(nport == 0 || (port && port_out), GG_EINVAL, "null port arrays");
    const int n = s->A.n;
    GG_REQUIRE(src_off[0] == 0, GG_EINVAL, "gg_transient_batch: src_off[0] != 0");
    for (int q = 0; q < nrhs; q++) GG_REQUIRE(src_off[q + 1] >= src_off[q], GG_EINVAL, "gg_transient_batch: src_off not monotone");
    const int ns = src_off[nrhs];
    GG_REQUIRE(ns == 0 || (src_node && src_kind && src_ptr && src_data), GG_EINVAL, "null source arrays");
    int maxsrc = 0;
    std::vector<int> kind(std::max(ns, 1), GG_SRC_DC), dptr(ns + 1, 0);
    for (int q = 0; q < nrhs; q++) maxsrc = std::max(maxsrc, src_off[q + 1] - src_off[q]);
    for (int k = 0; k < ns; k++) {
        GG_REQUIRE(src_node[k] >= 0 && src_node[k] < n, GG_EINVAL, "source node out of range");
        const int len = src_ptr[k + 1] - src_ptr[k];
        GG_REQUIRE(src_ptr[k] >= 0 && len >= 0, GG_EINVAL, "transient: bad src_ptr");
        const int need = src_kind[k] == GG_SRC_DC ? 1 : src_kind[k] == GG_SRC_PULSE ? 7 : -1;
        GG_REQUIRE(src_kind[k] == GG_SRC_DC || src_kind[k] == GG_SRC_PULSE || src_kind[k] == GG_SRC_PWL, GG_EINVAL,
                   "transient: unknown source kind");
        GG_REQUIRE(need < 0 ? (len >= 2 && len % 2 == 0) : len == need, GG_EINVAL,
                   "transient: DC takes 1 value, PULSE 7, PWL (time, value) pairs");
        kind[k] = src_kind[k];
        dptr[k + 1] = src_ptr[k + 1] - src_ptr[0];
    }
    for (int j = 0; j < nport; j++) GG_REQUIRE(port[j] >= 0 && port[j] < n, GG_EINVAL, "port out of range");
    // per scenario, B^T by row: the scenario's sources of each row in ascending
    // index (cs_dl_gaxpy's column order, as gg_transient)
    std::vector<int> sptr((size_t)nrhs * (n + 1), 0), sidx(std::max(ns, 1));
    for (int q = 0; q < nrhs; q++) {
        int *sp = sptr.data() + (size_t)q * (n + 1);
        for (int k = src_off[q]; k < src_off[q + 1]; k++) sp[src_node[k] + 1]++;
        sp[0] = src_off[q];
        for (int r = 0; r < n; r++) sp[r + 1] += sp[r];
        std::vector<int> fill(sp, sp + n);
        for (int k = src_off[q]; k < src_off[q + 1]; k++) sidx[fill[src_node[k]]++] = k;
    }
    GG_HIP(hipSetDevice(s->device));
    hipStream_t st = s->st;
    DBuf<int> d_soff, d_kind, d_dptr, d_sptr, d_sidx, d_port;
    DBuf<double> d_data, d_u, d_c, d_x, d_w, d_pv;
    d_soff.upload(src_off, nrhs + 1, st);
    d_kind.upload(kind, st);
    d_dptr.upload(dptr, st);
    d_data.upload(ns ? src_data + src_ptr[0] : cdiag, ns ? (size_t)(src_ptr[ns] - src_ptr[0]) : 1, st);
    d_sptr.upload(sptr, st);
    d_sidx.upload(sidx, st);
    d_u.alloc(std::max(ns, 1));
    d_c.upload(cdiag, n, st);
    d_x.upload(x, (size_t)nrhs * n, st);
    d_w.alloc((size_t)nrhs * n);
    d_port.upload(port, nport, st);
    const long long ldo = (long long)nport * (nsteps + 1);
    d_pv.alloc((size_t)std::max<long long>(ldo * nrhs, 1));
    launch_gather_ports_b(nport, d_port.p, d_x.p, n, d_pv.p, ldo, nrhs, st);
    std::vector<gg_result> res(nrhs);
    std::vector<long long> tot(nrhs, 0);
    int status = GG_OK;
    struct HintReset {
        gg_solver *s;
        ~HintReset() { s->batch_iter_hint = 0; }
    } hint_reset{s};
    s->batch_iter_hint = 0;
    for (int it = 1; it <= nsteps; it++) {
        launch_transient_step_b(n, nrhs, maxsrc, d_soff.p, d_kind.p, d_dptr.p, d_data.p, it, h, d_u.p, d_sptr.p,
                                d_sidx.p, d_c.p, d_x.p, d_w.p, n, st);
        const int rc = method == BATCH_CG         ? solve_cg_batch(s, nrhs, d_w.p, n, d_x.p, n, opt, res.data())
                       : method == BATCH_BICGSTAB ? solve_bicgstab_batch(s, nrhs, d_w.p, n, d_x.p, n, opt, res.data())
                                                  : solve_batch(s, nrhs, d_w.p, n, d_x.p, n, opt, res.data());
        if (rc < 0) return rc;
        if (rc) status = rc;
        for (int q = 0; q < nrhs; q++) tot[q] += res[q].iters;
        if (method != BATCH_GMRES) {
            int mx = 0;
            for (int q = 0; q < nrhs; q++) mx = std::max(mx, res[q].inner_iters);
            s->batch_iter_hint = mx;
        }
        launch_gather_ports_b(nport, d_port.p, d_x.p, n, d_pv.p + (long long)it * nport, ldo, nrhs, st);
    }
    if (nport) {
        std::vector<double> pv((size_t)ldo * nrhs);
        GG_HIP(hipMemcpyAsync(pv.data(), d_pv.p, pv.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        GG_HIP(hipStreamSynchronize(st));
        for (int q = 0; q < nrhs; q++)
            for (int it = 0; it <= nsteps; it++)
                for (int j = 0; j < nport; j++)
                    port_out[((size_t)q * nport + j) * (nsteps + 1) + it] = pv[(size_t)q * ldo + (size_t)it * nport + j];
    }
    GG_HIP(hipMemcpyAsync(x, d_x.p, (size_t)nrhs * n * sizeof(double), hipMemcpyDeviceToHost, st));
    GG_HIP(hipStreamSynchronize(st));
    for (int q = 0; q < nrhs; q++) iters_total[q] = (int)std::min<long long>(tot[q], INT32_MAX);
    return status;
}
