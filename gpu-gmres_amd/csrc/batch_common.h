// batch_common.h -- what the many-RHS solves share (batch.hip: GMRES,
// cg_batch.hip: CG, bicgstab_batch.hip: BiCGStab): the per-scenario arena, the ring of read-back slots, the
// triage of the error word, the staging around a solve and the host-array entry
// point.  A method keeps which arrays a scenario owns, the launches of an
// iteration or cycle, how a control block becomes a gg_result, and its fallbacks.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <deque>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "gg_api.h"
#include "gg_solver.h"

namespace gg {

// scenario q's copy of a per-scenario pointer
template <class T>
T *zq(T *p, long long zs, int q)
{
    return reinterpret_cast<T *>(reinterpret_cast<char *>(const_cast<typename std::remove_const<T>::type *>(p)) +
                                 (long long)q * zs);
}

// The arena: every per-scenario array of scenario 0 side by side, each 256-B
// aligned, zs bytes in all; scenario q's copy q * zs bytes further on.  A
// method names each array once, between begin and commit:
//     A.begin(s, S, hist_need, method);  A.take(x, P);  A.take(hist, A.hist_cap);  ...  A.commit(st);
// take notes where the scenario-0 pointer goes and commit fills it in.
struct BatchArena {
    int S = 0;
    long long zs = 0;                    // bytes per scenario
    DBuf<char> buf;
    // the reuse key beyond S: the vector space, the history's room, the solves'
    // granule counts, gg_set_matrix_count() when the arena was zeroed (a new
    // layout moves the padding, and the dots read whole units) and the method's
    // own integer (GMRES: the restart length)
    long long Ppad = 0, hist_cap = 0, ngL = 0, ngU = 0, matrix = -1, method = 0;
    unsigned long long *Lg = nullptr, *Ug = nullptr;     // the L and U solves' hand-off granules
    std::vector<long long> hist_len;     // per scenario, of the last batched solve

    bool fits(const gg_solver *s, int S_, long long hist_need, long long method_) const
    {
        return buf.p && S == S_ && method == method_ && Ppad == s->Ppad && hist_cap >= hist_need &&
               matrix == gg_set_matrix_count() && ngL == trsv_b_granules(s->L) && ngU == trsv_b_granules(s->U);
    }
    void begin(gg_solver *s, int S_, long long hist_need, long long method_)
    {
        GG_HIP(hipStreamSynchronize(s->st));            // nothing in flight reads the old one
        S = S_;
        method = method_;
        Ppad = s->Ppad;
        matrix = gg_set_matrix_count();
        hist_cap = std::max<long long>(hist_need, 64);
        ngL = trsv_b_granules(s->L);
        ngU = trsv_b_granules(s->U);
        hist_len.assign(S, 0);
        o = 0;
        binds.clear();
    }
    template <class T>
    void take(T *&at, long long count)
    {
        binds.emplace_back(&at, o);
        o = (o + count * (long long)sizeof(T) + 255) / 256 * 256;
    }
    void commit(hipStream_t st)
    {
        zs = o;
        buf.alloc((size_t)zs * S);
        // every vector +0 in its padding slots, every dummy granule 0 (read as ready)
        GG_HIP(hipMemsetAsync(buf.p, 0, (size_t)zs * S, st));
        for (const auto &[at, off] : binds) {
            char *p = buf.p + off;
            std::memcpy(at, &p, sizeof p);
        }
        binds.clear();
    }
    // scenario q's residual history (hist: scenario 0's) from the device
    long long history(const double *hist, int q, double *out, long long cap) const
    {
        GG_REQUIRE(q >= 0 && q < (int)hist_len.size() && hist_len[q] > 0, GG_ESTATE,
                   "gg_batch_history: no batched solve holds that scenario");
        const long long n = hist_len[q];
        if (out && cap > 0)
            GG_HIP(hipMemcpy(out, zq(hist, zs, q), std::min(n, cap) * sizeof(double), hipMemcpyDeviceToHost));
        return n;
    }

private:
    long long o = 0;
    std::vector<std::pair<void *, long long>> binds;     // (a scenario-0 pointer's place, its offset)
};

// The error word of a read-back: bit 0 a wavefront wait timed out (fatal, with
// the caller's text), bit 1 a WD_RCP range miss (the caller applies the
// Fallback -- IEEE division for the solver's life -- and repeats the solve)
inline void batch_triage(int err, const char *timeout_text)
{
    GG_REQUIRE((err & 1) == 0, GG_ETIMEOUT, timeout_text);
    if (err & 2) throw Fallback{err};
}

// The read-back ring: the scenarios' control blocks and, behind them, the
// error word, packed by k_pack_states_b straight into one of kSlots mapped
// pinned slots, then the slot's event.  The host enqueues a chunk ahead of what
// it has read, so posts queue up; they are waited for oldest first.
//
// When a slot may be written again: posts and their packs run in stream order,
// so a wait leaves its own and every earlier post finished; and the block a
// wait returns is read only until the next post (callers copy what they keep).
// The slots rotate, so with at most kSlots - 2 posts outstanding the slot of a
// new post is neither in flight nor the one read last.  post() requires that.
template <class State>
struct ReadRing {
    static constexpr int kSlots = 4;
    State *h[kSlots] = {};
    State *d[kSlots] = {};
    hipEvent_t ev[kSlots] = {};

    ReadRing() = default;
    ReadRing(const ReadRing &) = delete;
    ReadRing &operator=(const ReadRing &) = delete;
    ~ReadRing() { release(); }
    void release()
    {
        for (int k = 0; k < kSlots; k++) {
            if (h[k]) (void)hipHostFree(h[k]);
            if (ev[k]) (void)hipEventDestroy(ev[k]);
            h[k] = d[k] = nullptr;
            ev[k] = nullptr;
        }
    }
    void alloc(int S)
    {
        release();
        for (int k = 0; k < kSlots; k++) {
            GG_HIP(hipHostMalloc(reinterpret_cast<void **>(&h[k]), sizeof(State) * (size_t)(S + 1),
                                 hipHostMallocMapped));
            GG_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&d[k]), h[k], 0));
            GG_HIP(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
        }
    }
    // a solve starts: nothing posted, slot 0 next; st0 = scenario 0's control block
    void begin(gg_solver *s_, const BatchArena &A, const State *st0_, const char *timeout_text_)
    {
        s = s_;
        st0 = st0_;
        zs = A.zs;
        S = A.S;
        timeout_text = timeout_text_;
        next = 0;
        posted.clear();
    }
    void post(int tag = 0)
    {
        GG_REQUIRE((int)posted.size() <= kSlots - 2, GG_EHIP, "batched solve: read-back ring overrun");
        launch_pack_states_b(st0, zs, S, d[next], s->err.p, s->st);
        GG_HIP(hipEventRecord(ev[next], s->st));
        posted.emplace_back(next, tag);
        next = (next + 1) % kSlots;
    }
    bool pending() const { return !posted.empty(); }
    const State *wait_oldest(int *tag = nullptr)
    {
        const auto [k, t] = posted.front();
        posted.pop_front();
        if (tag) *tag = t;
        return wait(k);
    }
    // the state after everything enqueued so far, older posts forgotten (they
    // are finished when this one is)
    const State *post_and_wait()
    {
        post();
        return drain();
    }
    // the newest post, and with it every post (nullptr: nothing was posted)
    const State *drain()
    {
        if (posted.empty()) return nullptr;
        const int k = posted.back().first;
        posted.clear();
        return wait(k);
    }

private:
    const State *wait(int k)
    {
        GG_HIP(hipEventSynchronize(ev[k]));
        batch_triage(*reinterpret_cast<const int *>(h[k] + S), timeout_text);
        return h[k];
    }
    gg_solver *s = nullptr;
    const State *st0 = nullptr;
    long long zs = 0;
    int S = 0, next = 0;
    const char *timeout_text = "";
    std::deque<std::pair<int, int>> posted;     // (slot, the caller's tag), oldest first
};

// out = M in for every scenario: the L solve into t1, the U solve out of it
inline void batch_minv(gg_solver *s, const BatchArena &A, Gate g, const double *in, double *t1, double *out)
{
    launch_trsv_b(g, s->L, in, t1, A.Lg, s->err.p, A.S, A.zs, s->st);
    launch_trsv_b(g, s->U, t1, out, A.Ug, s->err.p, A.S, A.zs, s->st);
}

// A batched solve's prologue: b and x gathered into the solver's vector space
// (bv, xv: scenario 0's), the hand-off granules armed, the method's control
// blocks set (init_states, one launch), the error word cleared, ev0.
template <class Init>
void stage_in(gg_solver *s, const BatchArena &A, const double *d_b, long long ldb, const double *d_x, long long ldx,
              double *bv, double *xv, Init init_states)
{
    hipStream_t st = s->st;
    if (!s->err.p) s->err.alloc(1);
    launch_gather_b(d_b, ldb * 8, s->lay2nat.p, bv, A.zs, s->Ppad, A.S, st);
    launch_gather_b(d_x, ldx * 8, s->lay2nat.p, xv, A.zs, s->Ppad, A.S, st);
    launch_fill_u64(A.Lg, s->L.wl.ngran(), kSentinel, st, Batch{A.S, A.zs});
    launch_fill_u64(A.Ug, s->U.wl.ngran(), kSentinel, st, Batch{A.S, A.zs});
    init_states();
    GG_HIP(hipMemsetAsync(s->err.p, 0, sizeof(int), st));
    GG_HIP(hipEventRecord(s->ev0, st));
}

// The epilogue: ev1, x back to the caller's order, a last read-back for the
// error word after every launch (drained with whatever was still posted: the
// chunk behind the end, gated off).  Returns ev0 .. ev1 in ms.
template <class State>
float stage_out(gg_solver *s, const BatchArena &A, ReadRing<State> &ring, const double *xv, double *d_x, long long ldx)
{
    GG_HIP(hipEventRecord(s->ev1, s->st));
    launch_gather_b(xv, A.zs, s->nat2lay.p, d_x, ldx * 8, s->A.n, A.S, s->st);
    (void)ring.post_and_wait();
    float ms = 0.f;
    GG_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    return ms;
}

// The host-array entry points (gg_solve_batch, gg_solve_cg_batch,
// gg_solve_bicgstab_batch; name: the
// entry point's, for its messages): upload, the device engine, download.
// download_on_error: x is copied back whatever the engine returned; otherwise
// not after a negative code other than GG_EBREAKDOWN.
using BatchEngine = int (*)(gg_solver *, int, const double *, long long, double *, long long, const gg_options *,
                            gg_result *);
inline int solve_batch_host(gg_solver *s, BatchEngine engine, const char *name, bool download_on_error, int nrhs,
                            const double *b, long long ldb, double *x, long long ldx, const gg_options *opt,
                            gg_result *res)
{
    GG_REQUIRE(s && b && x, GG_EINVAL, "null argument");
    GG_REQUIRE(s->have_A, GG_ESTATE, std::string(name) + ": no matrix");
    GG_REQUIRE(nrhs >= 1 && ldb >= s->A.n && ldx >= s->A.n, GG_EINVAL,
               std::string(name) + ": bad nrhs / leading dimension");
    GG_HIP(hipSetDevice(s->device));
    const int n = s->A.n;
    DBuf<double> db, dx;
    db.alloc((size_t)nrhs * n);
    dx.alloc((size_t)nrhs * n);
    for (int q = 0; q < nrhs; q++) {
        GG_HIP(hipMemcpyAsync(db.p + (size_t)q * n, b + (size_t)q * ldb, n * sizeof(double), hipMemcpyHostToDevice, s->st));
        GG_HIP(hipMemcpyAsync(dx.p + (size_t)q * n, x + (size_t)q * ldx, n * sizeof(double), hipMemcpyHostToDevice, s->st));
    }
    const int rc = engine(s, nrhs, db.p, n, dx.p, n, opt, res);
    if (!download_on_error && rc < 0 && rc != GG_EBREAKDOWN) return rc;
    for (int q = 0; q < nrhs; q++)
        GG_HIP(hipMemcpyAsync(x + (size_t)q * ldx, dx.p + (size_t)q * n, n * sizeof(double), hipMemcpyDeviceToHost, s->st));
    GG_HIP(hipStreamSynchronize(s->st));
    return rc;
}

}  // namespace gg
