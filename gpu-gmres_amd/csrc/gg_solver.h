// gg_solver.h -- the single-device solver object behind the C ABI (solver.hip)
// and what its engines in other files declare to each other: the many-RHS
// batches (batch.hip: GMRES, cg_batch.hip: CG, bicgstab_batch.hip: BiCGStab; the
// arena, read-back ring and staging they share are batch_common.h's), the
// short-recurrence solves (cg.hip, bicgstab.hip) and the read-back pipe,
// error-word triage and fallback they all use.  The C ABI's exception boundary
// is gg_api.h.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "kernels.h"

namespace gg {
struct BatchWs;                       // batch.hip
void batch_release(gg_solver *s);     // frees s->batch (gg_destroy)
// solver.hip: one single-scenario device solve (gg_solve_device's engine, with
// its fallbacks) and the padding map of the solver's vector space
int solve_one(gg_solver *s, const double *d_b, double *d_x, const gg_options *opt, gg_result *res);
UnitMap solver_unit_map(const gg_solver *s);
// batch.hip: the many-RHS engine behind gg_solve_batch_device
int solve_batch(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                const gg_options *opt, gg_result *res);
bool batch_engine_on(gg_solver *s);
std::string batch_mgs_kernel(gg_solver *s);     // gg_batch_mgs_kernel
long long batch_history(gg_solver *s, int q, double *out, long long cap);
// cg_batch.hip: the many-RHS conjugate-gradient engine behind
// gg_solve_cg_batch_device (also the CG transient batch's step), its
// per-scenario histories (batch_history hands over when the last batch ran
// CG: s->batch_last) and its work space
struct CgBatchWs;
int solve_cg_batch(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                   const gg_options *opt, gg_result *res);
long long cg_batch_history(gg_solver *s, int q, double *out, long long cap);
void cg_batch_release(gg_solver *s);
// bicgstab_batch.hip: the same for BiCGStab, behind gg_solve_bicgstab_batch_device
struct BiBatchWs;
int solve_bicgstab_batch(gg_solver *s, int S, const double *d_b, long long ldb, double *d_x, long long ldx,
                         const gg_options *opt, gg_result *res);
long long bicgstab_batch_history(gg_solver *s, int q, double *out, long long cap);
void bicgstab_batch_release(gg_solver *s);
// the method of a batch: the last one's on the solver (s->batch_last;
// gg_batch_history and gg_batch_mgs_kernel read it), a transient's step
enum BatchMethod { BATCH_GMRES = 0, BATCH_CG = 1, BATCH_BICGSTAB = 2 };
// batch.hip: the body of gg_transient_batch, gg_transient_cg_batch and
// gg_transient_bicgstab_batch (method: the step's solver; CG's and BiCGStab's
// first chunk is sized by the previous step)
int transient_batch(gg_solver *s, BatchMethod method, int nrhs, int nsteps, double h, const double *cdiag,
                    const int *src_off, const int *src_node, const int *src_kind, const int *src_ptr,
                    const double *src_data, int nport, const int *port, double *x, const gg_options *opt,
                    double *port_out, int *iters_total);
// cg.hip, bicgstab.hip: the GG_SOLVE_CG and GG_SOLVE_BICGSTAB engines behind
// solve_device (arguments checked by the caller, s->shared set); both are
// short_recurrence.h's driver over their own launches
int solve_cg(gg_solver *s, const double *d_b, double *d_x, const gg_options *opt, gg_result *res);
int solve_bicgstab(gg_solver *s, const double *d_b, double *d_x, const gg_options *opt, gg_result *res);
// solver.hip, shared with short_recurrence.h.  Fallback: a wavefront solve asked
// for a repeat on its safe path (the error word's bits 1 and 3); solve_device
// applies it and starts the solve over
struct Fallback {
    int bits;
};
// The device error word (solver.hip check_err) into the throw or the raise, in
// this order: bit 3 -> Fallback, bit 0 -> GG_ETIMEOUT, bit 1 -> Fallback.
// Returns when none of kErrSolve is set.
constexpr int kErrSolve = 8 | 1 | 2;
void raise_err(int err);
// for the rest of the solver's life: every WD_RCP triangle divides (bit 1),
// every 3D tile triangle claims its tiles from the queue (bit 3)
void apply_fallback(gg_solver *s, const Fallback &f);
// The read-back pipe (solver.hip): a solve enqueues work one unit (a restart
// cycle, a chunk of iterations) ahead of the state the host has read.  Each
// unit ends in a post: the control block and the error word copied into one of
// two pinned slots, then an event.  A solver runs one solve at a time, so one
// pipe serves GMRES, CG and BiCGStab.
struct ReadPipe {
    void *state[2] = {nullptr, nullptr};    // kPipeSlotBytes each
    int *err[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::vector<size_t> mark_ends;          // marks.size() after each posted unit not yet collected
};
constexpr size_t kPipeSlotBytes = std::max({sizeof(DevState), sizeof(CgState), sizeof(BiState)});
void pipe_begin(gg_solver *s);              // slots and events allocated once; nothing posted
// the state (bytes at dev_state) and the error word into the slot, then its
// event; close_marks: the profile marks enqueued so far end a unit here
void pipe_post(gg_solver *s, int slot, const void *dev_state, size_t bytes, bool close_marks = true);
int pipe_wait(gg_solver *s, int slot);      // the slot's error word; its state: pipe_state (below)
void pipe_collect(gg_solver *s, int executed);      // the oldest posted unit's marks
void pipe_drain(gg_solver *s);              // waits for the unit behind the last (gated off), drops its marks
void pipe_release(gg_solver *s);            // gg_destroy
// the Ppad-long work vectors, partials, control block, error word; bicgstab: also the
// three vectors that solve alone keeps (bi_rt, bi_t, bi_q)
void ensure_vectors(gg_solver *s, bool bicgstab = false);
void zero_vectors(gg_solver *s);            // those vectors back to +0, padding included
void apply_minv(gg_solver *s, Gate g, const double *in, double *out, int i = -1);   // out = M in
void reset_wave(DevTri *T, hipStream_t st);
void check_err(gg_solver *s);
int prof_begin(gg_solver *s, int kind, int i);
void prof_end(gg_solver *s, int mark);
void prof_collect(gg_solver *s, int executed, size_t upto = (size_t)-1);
}  // namespace gg

using gg::Csr;
using gg::DBuf;
using gg::DevCsr;
using gg::DevState;
using gg::DevTri;
using gg::Wave2D;

struct gg_solver {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    Csr A;
    bool have_A = false;
    int pkind = -1;       // -1: not set

    // vector space (natural or wavefront layout)
    bool wave = false;
    bool relabeled = false;   // off the wavefront, an RCM layout (setup_space)
    Wave2D wl;
    long long P = 0, Ppad = 0;
    std::vector<long long> nat2lay_h;
    DBuf<long long> lay2nat, nat2lay;
    int G = 1;

    DevCsr dA;            // A in layout space (split: A' -- rows in prow order, columns by pcol)
    DevTri L, U;
    // Split (PG) engine, every vector in the triangles' layout (natural or
    // wavefront).  With lay = the layout map of the triangles' row space:
    //   A'  row lay(j) = A row prow[j], column c -> lay(pcol[c])
    //   mid_l[lay(r)] = middle[r], ls_l[lay(j)] = lscale[prow[j]],
    //   rs_l[lay(r)] = rscale[pcol^-1[r]]   (all three 1.0 in padding slots)
    // so that Ml(A Mr(v)) = L^-1 (A' (U^-1 (mid_l o v) / rs_l)) / ls_l with the
    // row gather, the column scatter and both scalings folded into the SpMV's
    // indices and epilogue and the U solve's store (each value rounded by the
    // same operation as in MyILUPPfloat::DevPrecond_*, src/preconditioner.cu:
    // 1424-1657).  x lives in the same column convention: x[c] at lay(pcol[c]).
    DBuf<double> mid_l, ls_l, rs_l;
    // stage maps (layout slot -> natural index, -1 = padding): b in A' row
    // order, x in the column convention; and back: x_out[c] = lay(pcol[c]),
    // y_out[r] = lay(prow^-1[r])
    DBuf<long long> sb_map, sx_map, sx_out, sy_out;
    DevCsr dUfull;        // the split U factor (diagonal first) in layout space (apply_start)
    // AINV / DIAG (gg_set_precond_ainv / _diag; natural order): M = Wt diag(dinv) Z
    // applied as two products; DIAG keeps its reciprocals in ainv_d
    DevCsr aZ, aWt;
    DBuf<double> ainv_d;
    double ainv_bytes = 0;              // algorithmic bytes per application
    long long ainv_nnz[2] = {0, 0};     // nnz(Z), nnz(Wt)
    // caller-supplied preconditioner (gg_set_precond_user): fp32 staging of its
    // device arrays, natural order
    gg_precond_fn ufn = nullptr;
    void *uctx = nullptr;
    DBuf<float> fin, fout;

    // workspace
    int m_alloc = -1;
    bool vec_ok = false;  // the work vectors below are allocated for this space (ensure_vectors)
    DBuf<double> V, w, ww, r, rr, bb, t1, t2, z, xv, bv, y;
    DBuf<double> partA, partB, H, s, cs, sn, ysm;
    // persistent Arnoldi orthogonalization (kernels/arnoldi_persist.hip k_arnoldi_persist)
    bool persist = false;
    bool split_local = false;   // the split engine's vectors in a local layout (grid / RCM): its gathers are near
    bool wide = false;                  // k_arnoldi_wide (vectors beyond persist's registers)
    bool shared = false;                // GG_SOLVE_SHARED_DEVICE for the solve in progress
    int div_mode = GG_DIV_EXACT;        // gg_set_division: the wavefront solves' division
    gg::ReadPipe pipe;                  // pinned read-backs of the control block and the error word
    int resid_fallbacks = 0;            // cycles rerun after a persistent grid was not co-resident
    int iter_hint = 0;                  // transient loop: the previous step's inner iterations (0: none)
    // GG_SOLVE_CG and GG_SOLVE_BICGSTAB (short_recurrence.h): the control blocks and the
    // dots' block partials (1024 each; cg.hip: p.q | r.z, z.z; bicgstab.hip: rt.v | t.s, t.t |
    // r.r, rt.r)
    DBuf<gg::CgState> cgs;
    DBuf<gg::BiState> bis;
    DBuf<double> sr_part;
    bool last_cg = false;               // the last solve ran CG or BiCGStab (gg_mgs_kernel: no orthogonalization)
    // BiCGStab's vectors beyond the GMRES work space (the shadow residual, t, the
    // SpMV output M is applied to)
    DBuf<double> bi_rt, bi_t, bi_q;
    bool bi_vec_ok = false;
    // transient tap-node statistics (gg_transient_set_taps / _get_taps)
    std::vector<int> taps;
    std::vector<double> tap_max, tap_min, tap_avg;
    DBuf<unsigned long long> gran;      // m * (m+2) * G hand-off granules, then m * (m+2) sums
                                        // (gather_h), re-armed per cycle
    DBuf<unsigned long long> xgran;     // m * (m+2) * kMgsXcdWords: the XCD-local gather's slots (re-armed per cycle)
    DBuf<unsigned long long> elect;     // per XCD: the last launch that elected its reducer
    unsigned long long mgs_seq = 0;     // persistent orthogonalization launches so far (election)
    DBuf<long long> mgs_trace;          // diagnostics: GG_MGS_TRACE=N stamps the N-th persistent launch
    int mgs_trace_i = -1;               // (its inner index; printed to stderr after the solve)
    DBuf<double> hist;
    long long hist_cap = 0;
    DBuf<DevState> ds;
    DBuf<int> err;
    DBuf<double> nat_in, nat_out;   // staging for host-vector entry points
    std::vector<double> last_hist;

    // in-solve kernel timing (gg_profile_*)
    int prof_mask = 0;                  // (1 << GG_PROF_*) bits being timed
    std::vector<hipEvent_t> prof_pool;
    size_t prof_used = 0;
    std::vector<int> prof_free;         // pool slots of collected marks, reusable
    struct Mark { int kind, i, e0, e1; };
    std::vector<Mark> marks;
    double prof_ms[GG_PROF_NKINDS] = {};
    long long prof_cnt[GG_PROF_NKINDS] = {};

    // the many-RHS solve's per-scenario arenas (batch.hip), kept between
    // batched solves of the same shape
    gg::BatchWs *batch = nullptr;
    // the CG batch's (cg_batch.hip) and the BiCGStab batch's (bicgstab_batch.hip);
    // batch_last: the last batch's method, gg_batch_history reads it;
    // batch_iter_hint: the CG or BiCGStab transient batch's previous step, the
    // largest count of its scenarios (0: none)
    gg::CgBatchWs *cg_batch = nullptr;
    gg::BiBatchWs *bi_batch = nullptr;
    gg::BatchMethod batch_last = gg::BATCH_GMRES;
    int batch_iter_hint = 0;
};

namespace gg {
// the state a post copied into the slot (after pipe_wait)
template <class State>
const State &pipe_state(const gg_solver *s, int slot)
{
    return *static_cast<const State *>(s->pipe.state[slot]);
}
}  // namespace gg
