// cg_batch.hip -- the many-RHS conjugate-gradient solve: nrhs independent
// right-hand sides on ONE matrix and preconditioner, every launch of a CG
// iteration serving all scenarios (DESIGN.md "CG batch").
//
// The method is cg.hip's, the batch is batch.hip's: scenario q keeps its own
// vectors, partials, control block (CgState) and history in an arena of its
// own, q * zs bytes after scenario 0's, and an iteration is seven launches for
// all scenarios together --
//   launch_spmv_b     q = A p         (A's entries read once per 8 scenarios)
//   launch_cg_pq_b    partials of p . q
//   launch_cg_xr_b    alpha; x = alpha p + x; r = (-alpha) q + r
//   launch_trsv_b L, U   z = M r      (one wavefront dependency chain for all)
//   launch_cg_rz_b    partials of r . z and z . z
//   launch_cg_p_b     res, beta; p = beta p + z
// Per scenario the arithmetic is the single solve's -- the same kernels with a
// scenario offset -- so scenario q's status, count, history and solution are
// bit-identical to gg_solve_device(GG_SOLVE_CG) on that right-hand side alone.
// A scenario whose gate is closed (converged, converged at the start, broken
// down, max_iter reached) drops out of every launch; the others go on.
//
// Iterations are enqueued in chunks with the host one chunk ahead of the
// control blocks it has read (k_pack_cg_states_b into mapped pinned slots, as
// the GMRES batch); there is no host synchronization per iteration.  The
// batch ends when a read-back shows every scenario over; the launches enqueued
// behind that point are gated off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <string>
#include <vector>

#include "gg_solver.h"

namespace gg {

// Per-scenario arena (offsets in bytes, each 256-B aligned), the read-back
// slots, and the histories of a scenario-by-scenario run.
struct CgBatchWs {
    int S = 0;
    long long Ppad = 0, hist_cap = 0, ngL = 0, ngU = 0;
    long long matrix = -1;               // gg_set_matrix_count() when the arena was zeroed (a new layout moves the padding)
    long long zs = 0;                    // bytes per scenario
    DBuf<char> arena;
    long long ox = 0, ob = 0, or_ = 0, oz = 0, op = 0, oq = 0, obb = 0, ot1 = 0, opart = 0, ocs = 0, ohist = 0,
              oLg = 0, oUg = 0;
    // read-back slots: S control blocks, then the error word
    static constexpr int kSlots = 4;
    CgState *h_st[kSlots] = {};
    CgState *d_st[kSlots] = {};
    hipEvent_t ev[kSlots] = {};
    // the last solve's histories: lengths in the arena (batched), or the
    // vectors themselves (scenario by scenario)
    bool seq = false;
    std::vector<long long> hist_len;
    std::vector<std::vector<double>> seq_hist;
    double *dp(long long off) { return reinterpret_cast<double *>(arena.p + off); }
    void free_slots()
    {
        for (int k = 0; k < kSlots; k++) {
            if (h_st[k]) (void)hipHostFree(h_st[k]);
            if (ev[k]) (void)hipEventDestroy(ev[k]);
            h_st[k] = d_st[k] = nullptr;
            ev[k] = nullptr;
        }
    }
    ~CgBatchWs() { free_slots(); }
};

void cg_batch_release(gg_solver *s)
{
    delete s->cg_batch;
    s->cg_batch = nullptr;
}

namespace {

constexpr long long kAlign = 256;
long long align_up(long long a) { return (a + kAlign - 1) / kAlign * kAlign; }

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
    if (B->arena.p && B->S == S && B->Ppad == s->Ppad && B->hist_cap >= hist_need &&
        B->matrix == gg_set_matrix_count() && B->ngL == trsv_b_granules(s->L) && B->ngU == trsv_b_granules(s->U))
        return;
    GG_HIP(hipStreamSynchronize(s->st));
    B->free_slots();
    B->S = S;
    B->Ppad = s->Ppad;
    B->matrix = gg_set_matrix_count();
    B->hist_cap = std::max<long long>(hist_need, 64);
    B->ngL = trsv_b_granules(s->L);
    B->ngU = trsv_b_granules(s->U);
    const long long P = s->Ppad;
    long long o = 0;
    auto take = [&](long long bytes) {
        const long long at = o;
        o = align_up(o + bytes);
        return at;
    };
    B->ox = take(P * 8);
    B->ob = take(P * 8);
    B->or_ = take(P * 8);
    B->oz = take(P * 8);
    B->op = take(P * 8);
    B->oq = take(P * 8);
    B->obb = take(P * 8);
    B->ot1 = take(P * 8);
    B->opart = take(3 * 1024 * 8);       // p.q | r.z, z.z (cg.hip)
    B->ocs = take((long long)sizeof(CgState));
    B->ohist = take(B->hist_cap * 8);
    B->oLg = take(B->ngL * 8);
    B->oUg = take(B->ngU * 8);
    B->zs = align_up(o);
    B->arena.alloc((size_t)B->zs * S);
    // every vector +0 in its padding slots, every dummy granule 0 (read as ready)
    GG_HIP(hipMemsetAsync(B->arena.p, 0, (size_t)B->zs * S, s->st));
    const size_t slot_bytes = sizeof(CgState) * (size_t)(S + 1);
    for (int k = 0; k < CgBatchWs::kSlots; k++) {
        GG_HIP(hipHostMalloc(reinterpret_cast<void **>(&B->h_st[k]), slot_bytes, hipHostMallocMapped));
        GG_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&B->d_st[k]), B->h_st[k], 0));
        GG_HIP(hipEventCreateWithFlags(&B->ev[k], hipEventDisableTiming));
    }
}

struct Ctx {
    gg_solver *s;
    CgBatchWs *B;
    int S, G;
    long long P, zs;
    CgState *cs;
    double *x, *b, *r, *z, *p, *q, *bb, *t1, *part, *hist;
    unsigned long long *Lg, *Ug;
};

// the scenarios' control blocks and the error word into read-back slot k, then its event
void readback(const Ctx &c, int k)
{
    launch_pack_cg_states_b(c.cs, c.zs, c.S, c.B->d_st[k], c.s->err.p, reinterpret_cast<int *>(c.B->d_st[k] + c.S),
                            c.s->st);
    GG_HIP(hipEventRecord(c.B->ev[k], c.s->st));
}

struct RangeMiss {};      // a WD_RCP step saw a numerator outside its safe range
// wait for slot k; the error word: bit 0 time-out (fatal), bit 1 a WD_RCP range
// miss (the caller repeats the solve with IEEE division)
const CgState *wait_slot(const Ctx &c, int k)
{
    GG_HIP(hipEventSynchronize(c.B->ev[k]));
    const int err = *reinterpret_cast<const int *>(c.B->h_st[k] + c.S);
    GG_REQUIRE((err & 1) == 0, GG_ETIMEOUT, "batched CG solve: wavefront boundary wait timed out");
    if (err & 2) throw RangeMiss{};
    return c.B->h_st[k];
}

void minv_b(const Ctx &c, Gate g, const double *in, double *out)
{
    gg_solver *s = c.s;
    launch_trsv_b(g, s->L, in, c.t1, c.Lg, s->err.p, c.S, c.zs, s->st);
    launch_trsv_b(g, s->U, c.t1, out, c.Ug, s->err.p, c.S, c.zs, s->st);
}

// Cg::enqueue_start for every scenario
void enqueue_start_b(const Ctx &c)
{
    gg_solver *s = c.s;
    const Gate none;
    minv_b(c, none, c.b, c.bb);                                                    // bb = M b
    launch_dot_b(none, c.bb, c.bb, c.part, c.G, c.P, c.S, c.zs, s->st);
    launch_normb_b(c.part, c.G, &c.cs->normb, c.S, c.zs, s->st);
    launch_spmv_b(none, s->dA, c.x, c.b, c.r, true, c.S, c.zs, s->st);              // r = b - A x
    minv_b(c, none, c.r, c.z);                                                     // z = M r
    launch_cg_rz_b(none, c.r, c.z, c.part + 1024, c.G, c.P, c.S, c.zs, s->st);
    launch_cg_p_b(none, 0, true, c.cs, c.part + 1024, c.G, c.p, c.z, c.hist, c.P, c.S, c.zs, s->st);   // p = z
}

// Cg::enqueue_iterations for every scenario, each launch gated per scenario
void enqueue_iterations_b(const Ctx &c, int k0, int k1)
{
    gg_solver *s = c.s;
    for (int k = k0; k < k1; k++) {
        Gate g;
        g.done = &c.cs->done;
        g.mask = ~0;
        g.nit = &c.cs->max_iter;
        g.i = k;
        launch_spmv_b(g, s->dA, c.p, nullptr, c.q, false, c.S, c.zs, s->st);        // q = A p
        launch_cg_pq_b(g, c.p, c.q, c.part, c.G, c.P, c.S, c.zs, s->st);
        launch_cg_xr_b(g, k, c.cs, c.part, c.G, c.x, c.p, c.r, c.q, c.P, c.S, c.zs, s->st);
        minv_b(c, g, c.r, c.z);                                                    // z = M r
        launch_cg_rz_b(g, c.r, c.z, c.part + 1024, c.G, c.P, c.S, c.zs, s->st);
        launch_cg_p_b(g, k, false, c.cs, c.part + 1024, c.G, c.p, c.z, c.hist, c.P, c.S, c.zs, s->st);
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
    CgBatchWs *B = s->cg_batch;
    if (!s->err.p) s->err.alloc(1);
    Ctx c;
    c.s = s;
    c.B = B;
    c.S = S;
    c.G = s->G;
    c.P = s->Ppad;
    c.zs = B->zs;
    c.cs = reinterpret_cast<CgState *>(B->arena.p + B->ocs);
    c.x = B->dp(B->ox);
    c.b = B->dp(B->ob);
    c.r = B->dp(B->or_);
    c.z = B->dp(B->oz);
    c.p = B->dp(B->op);
    c.q = B->dp(B->oq);
    c.bb = B->dp(B->obb);
    c.t1 = B->dp(B->ot1);
    c.part = B->dp(B->opart);
    c.hist = B->dp(B->ohist);
    c.Lg = reinterpret_cast<unsigned long long *>(B->arena.p + B->oLg);
    c.Ug = reinterpret_cast<unsigned long long *>(B->arena.p + B->oUg);
    hipStream_t st = s->st;

    // inputs into the solver's vector space; hand-off granules armed; control blocks
    launch_gather_b(d_b, ldb * 8, s->lay2nat.p, c.b, c.zs, c.P, S, st);
    launch_gather_b(d_x, ldx * 8, s->lay2nat.p, c.x, c.zs, c.P, S, st);
    launch_fill_u64_b(c.Lg, s->L.wl.ngran(), kSentinel, S, c.zs, st);
    launch_fill_u64_b(c.Ug, s->U.wl.ngran(), kSentinel, S, c.zs, st);
    launch_init_cg_state_b(c.cs, c.zs, S, opt->tol, max_iter, st);
    GG_HIP(hipMemsetAsync(s->err.p, 0, sizeof(int), st));
    GG_HIP(hipEventRecord(s->ev0, st));
    enqueue_start_b(c);

    // chunks of iterations, the host one chunk ahead (short_recurrence.h): chunk
    // c + 1 goes in before the control blocks after chunk c are read.  In a
    // transient the first chunk is the previous step's largest count + 2
    const int K = cg_batch_chunk();
    std::deque<int> pend;                               // read-back slots in flight, oldest first
    int slot = 0, next = 0;                             // next: first iteration not yet enqueued
    auto enqueue = [&](int len) {
        const int k1 = (int)std::min<long long>((long long)next + len, max_iter);
        enqueue_iterations_b(c, next, k1);
        next = k1;
        const int k = slot;
        slot = (slot + 1) % CgBatchWs::kSlots;
        readback(c, k);
        pend.push_back(k);
    };
    enqueue(s->batch_iter_hint > 0 ? s->batch_iter_hint + 2 : K);
    enqueue(K);
    std::vector<CgState> hs(S);
    while (true) {
        const int k = pend.front();
        pend.pop_front();
        const CgState *h = wait_slot(c, k);
        bool over = true;
        for (int q = 0; q < S; q++) over = over && (h[q].done || h[q].it >= max_iter);
        if (over) {
            std::copy(h, h + S, hs.begin());
            break;
        }
        enqueue(K);
    }
    GG_HIP(hipEventRecord(s->ev1, st));
    launch_gather_b(c.x, c.zs, s->nat2lay.p, d_x, ldx * 8, s->A.n, S, st);
    {
        // the chunk behind the end (gated off) and the error word after every launch
        const int k = slot;
        readback(c, k);
        pend.push_back(k);
        while (!pend.empty()) {
            (void)wait_slot(c, pend.front());
            pend.pop_front();
        }
    }
    float ms = 0.f;
    GG_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    std::vector<gg_result> out(S);
    B->seq = false;
    B->hist_len.assign(S, 0);
    for (int q = 0; q < S; q++) {
        const CgState &h = hs[q];
        B->hist_len[q] = (long long)h.it + 1;
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
    s->batch_last_cg = true;
    if (!batch_engine_on(s)) return solve_cg_batch_seq(s, S, d_b, ldb, d_x, ldx, opt, res);
    for (int attempt = 0;; attempt++) {
        try {
            return solve_cg_batch_once(s, S, d_b, ldb, d_x, ldx, opt, res);
        } catch (RangeMiss &) {
            // IEEE division for the solver's life, repeat (d_x is written only at the end)
            GG_HIP(hipStreamSynchronize(s->st));
            if (attempt >= 2) throw Error{GG_EHIP, "gg_solve_cg_batch: fallbacks exhausted"};
            for (DevTri *T : {&s->L, &s->U})
                if (T->kind == DevTri::WAVE2D && T->div == WD_RCP) T->div = WD_HW;
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
    GG_REQUIRE(q >= 0 && q < (int)B->hist_len.size() && B->hist_len[q] > 0, GG_ESTATE,
               "gg_batch_history: no batched solve holds that scenario");
    const long long n = B->hist_len[q];
    if (out && cap > 0)
        GG_HIP(hipMemcpy(out, B->arena.p + (long long)q * B->zs + B->ohist, std::min(n, cap) * sizeof(double),
                         hipMemcpyDeviceToHost));
    return n;
}

}  // namespace gg

// ======================================================================= C ABI
namespace {
int fail_cb(const gg::Error &e)
{
    gg::set_error(e.msg);
    return e.code;
}
}  // namespace
#define GG_CBAPI_BEGIN try {
#define GG_CBAPI_END                                                                 \
    }                                                                                \
    catch (const gg::Error &e) { return fail_cb(e); }                                \
    catch (const std::bad_alloc &) { return fail_cb({GG_ENOMEM, "host allocation failed"}); } \
    catch (const std::exception &e) { return fail_cb({GG_EINVAL, e.what()}); }

using namespace gg;

extern "C" {

int gg_solve_cg_batch_device(gg_solver *s, int nrhs, const double *d_b, long long ldb, double *d_x, long long ldx,
                             const gg_options *opt, gg_result *res)
{
    GG_CBAPI_BEGIN
    GG_REQUIRE(s && d_b && d_x, GG_EINVAL, "null argument");
    return solve_cg_batch(s, nrhs, d_b, ldb, d_x, ldx, opt, res);
    GG_CBAPI_END
}

int gg_solve_cg_batch(gg_solver *s, int nrhs, const double *b, long long ldb, double *x, long long ldx,
                      const gg_options *opt, gg_result *res)
{
    GG_CBAPI_BEGIN
    GG_REQUIRE(s && b && x, GG_EINVAL, "null argument");
    GG_REQUIRE(s->have_A, GG_ESTATE, "gg_solve_cg_batch: no matrix");
    GG_REQUIRE(nrhs >= 1 && ldb >= s->A.n && ldx >= s->A.n, GG_EINVAL,
               "gg_solve_cg_batch: bad nrhs / leading dimension");
    GG_HIP(hipSetDevice(s->device));
    const int n = s->A.n;
    DBuf<double> db, dx;
    db.alloc((size_t)nrhs * n);
    dx.alloc((size_t)nrhs * n);
    for (int q = 0; q < nrhs; q++) {
        GG_HIP(hipMemcpyAsync(db.p + (size_t)q * n, b + (size_t)q * ldb, n * sizeof(double), hipMemcpyHostToDevice, s->st));
        GG_HIP(hipMemcpyAsync(dx.p + (size_t)q * n, x + (size_t)q * ldx, n * sizeof(double), hipMemcpyHostToDevice, s->st));
    }
    const int rc = solve_cg_batch(s, nrhs, db.p, n, dx.p, n, opt, res);
    if (rc < 0 && rc != GG_EBREAKDOWN) return rc;
    for (int q = 0; q < nrhs; q++)
        GG_HIP(hipMemcpyAsync(x + (size_t)q * ldx, dx.p + (size_t)q * n, n * sizeof(double), hipMemcpyDeviceToHost, s->st));
    GG_HIP(hipStreamSynchronize(s->st));
    return rc;
    GG_CBAPI_END
}

int gg_transient_cg_batch(gg_solver *s, int nrhs, int nsteps, double h, const double *cdiag, const int *src_off,
                          const int *src_node, const int *src_kind, const int *src_ptr, const double *src_data,
                          int nport, const int *port, double *x, const gg_options *opt, double *port_out,
                          int *iters_total)
{
    GG_CBAPI_BEGIN
    return transient_batch(s, true, nrhs, nsteps, h, cdiag, src_off, src_node, src_kind, src_ptr, src_data, nport,
                           port, x, opt, port_out, iters_total);
    GG_CBAPI_END
}

}  // extern "C"
