/*
 * ggmres_dd.h -- C ABI of the sharded (domain-decomposed) solve, SURVEY.md 8(e):
 * GMRES(m), conjugate gradients (GG_SOLVE_CG, below), or BiCGStab through entry
 * points of its own (gg_dd_solve_bicgstab, below).
 *
 * Replaces the reference's multi-domain path: partition4 (src/partition3.cpp:122-194,
 * METIS_PartGraphRecursive -> our recursive BFS bisection / contiguous blocks),
 * dd_form's arrow-matrix blocks (src/form_dd.cpp:32-110) and the per-domain
 * solves of etbr_dd (src/etbr_dd.cpp), here as ONE GMRES(m) + ILU(0) solve of
 * the arrow-permuted system B = P A P^T sharded over nparts GPUs:
 *
 *   - shard p holds interior p's rows and a replica of the separator rows;
 *   - SpMV and the forward triangular solve need the "interface" values
 *     (interior nodes the separator rows reference) of every shard: one
 *     all-gather each (RCCL over xGMI); the backward solve needs nothing;
 *   - every MGS dot is an all-gather of the shards' block partials, summed in
 *     one fixed order on every shard (identical Hessenberg on every shard);
 *   - the ILU(0) factors are those of B (factored on the host), and each row
 *     of every triangular solve runs the reference's operations in the
 *     reference's order (LUSolve_ignoreZero, src/SpMV_compute.cpp:92-136):
 *     the operators are bit-identical to the single-GPU solve of B.
 *
 * Methods (opt->flags of gg_dd_solve / gg_dd_solve_device; every communicator):
 *   0              GMRES(m) with the reference's modified Gram-Schmidt;
 *   GG_SOLVE_CGS2  GMRES(m) with CGS2: three all-gathers per inner iteration;
 *   GG_SOLVE_CG    ggmres.h's GG_SOLVE_CG exactly, on B with M = the sharded
 *                  ILU(0) apply (symmetric where B is): no basis, no Hessenberg,
 *                  two all-gathers of dot partials per iteration whatever its
 *                  number -- p.q's, and ONE that carries r.z and z.z together.
 *                  tol, max_iter and restart as there (restart validated in
 *                  [1, 512], otherwise ignored; no Krylov work space is
 *                  allocated or touched).  gg_result: iters = inner_iters = the
 *                  iterations performed, restarts = 0, relres = the last
 *                  ||z|| / normb; gg_dd_get_history: the initial value, then
 *                  one entry per iteration.  GG_EBREAKDOWN when p.Ap is not
 *                  > 0, or r.Mr is not > 0 while the solve has not converged
 *                  (NaN counts as not > 0): x then holds the last iterate on
 *                  the rows this process owns, gg_last_error the text, and the
 *                  object is clean for the next solve.  The host enqueues the
 *                  iterations in chunks, one chunk ahead of the control block
 *                  it has read: one host wait per chunk, none per iteration.
 *   Any other combination is GG_EINVAL: GG_SOLVE_CG with GG_SOLVE_CGS2 (CG
 *   orthogonalizes nothing), and GG_SOLVE_BICGSTAB, which the sharded solve
 *   does not offer through these entry points: gg_dd_solve, gg_dd_solve_device,
 *   gg_dd_transient_src and gg_dd_transient answer it with GG_EINVAL, as they
 *   always have -- callers and tests rely on that refusal -- so sharded BiCGStab
 *   has a door of its own, gg_dd_solve_bicgstab and its kin below, named as the
 *   batches are (gg_solve_bicgstab_batch, gg_transient_bicgstab_batch).
 *
 * Three communicators:
 *   GG_DD_RCCL   one process per GPU (torchrun), shard = rank, RCCL collectives
 *                on the solver's stream; the 128-byte id comes from
 *                gg_dd_unique_id on rank 0 and is broadcast by the caller.
 *   GG_DD_IPC    one process per shard, device-initiated exchanges: every
 *                rank's exchange area (uncached device memory) is mapped into
 *                every process (hipIpc; over xGMI between GPUs) and each
 *                all-gather is ONE small kernel that stores this rank's slot
 *                into every peer's area and waits on the peers' sequence-
 *                numbered flags -- no collective library.  Several ranks may
 *                share a GPU (the one-GPU test of the multi-process path).
 *                Bootstrap: gg_dd_create, gg_dd_ipc_handle, the caller
 *                all-gathers the nparts handles (any host channel), then
 *                gg_dd_ipc_connect before gg_dd_set_system.
 *   GG_DD_LOCAL  all nparts shards in this process on one device (the same
 *                kernels, the exchanges done by a copy kernel): tests and
 *                single-GPU studies of the decomposition.
 *
 * Vectors are global, natural (unpermuted) order, length n, identical on every
 * rank on input.  On output a process writes the rows it holds (GG_DD_LOCAL:
 * all rows; GG_DD_RCCL / GG_DD_IPC: interior p and the separator); other
 * entries are left untouched.  Status codes as ggmres.h; GG_ECOMM for RCCL
 * failures, GG_ETIMEOUT when an IPC peer does not arrive within 30 s.
 */
#ifndef GGMRES_DD_H_
#define GGMRES_DD_H_

#include "ggmres.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GG_DD_ID_BYTES 128

#define GG_DD_IPC_HANDLE_BYTES 64

enum gg_dd_comm {
    GG_DD_LOCAL = 0,
    GG_DD_RCCL = 1,
    GG_DD_IPC = 2,
    /* timing only: ONE process holds shard `rank` of nparts and every exchange
     * is the in-process all-gather kernel over its own buffer (the other
     * shards' slots keep stale values) -- the per-rank kernel and exchange-launch
     * time of a one-shard-per-GPU run on this device alone.  The solve's values
     * are NOT the system's: run it for a fixed iteration count. */
    GG_DD_LOOPBACK = 3
};

typedef struct gg_dd gg_dd;

/* ncclGetUniqueId: call on rank 0, broadcast the bytes to every rank */
int gg_dd_unique_id(unsigned char *id);
int gg_dd_create(int device, int nparts, int comm, int rank, const unsigned char *id, gg_dd **out);
int gg_dd_destroy(gg_dd *d);
/* GG_DD_IPC: this rank's exchange-area handle (GG_DD_IPC_HANDLE_BYTES) ... */
int gg_dd_ipc_handle(gg_dd *d, unsigned char *handle);
/* ... and every rank's, rank-major (nparts * GG_DD_IPC_HANDLE_BYTES): maps the
 * peers' areas; returns once every rank has connected */
int gg_dd_ipc_connect(gg_dd *d, const unsigned char *handles);
/* processes in the exchange: GG_DD_RCCL the communicator's rank count
 * (ncclCommCount), GG_DD_IPC the mapped areas (checked: every rank reports
 * its own rank), GG_DD_LOCAL 1; *rank = this process's rank */
int gg_dd_comm_ranks(gg_dd *d, int *ranks, int *rank);

/* the global system (identical on every rank): partition (gg_part_method of
 * ggmres_host.h), arrow permutation, ILU(0) of the permuted matrix, shards */
int gg_dd_set_system(gg_dd *d, int n, const int *row_ptr, const int *col_idx, const double *val,
                     int method);
/* info[0..9] (exactly 10 ints): n, nparts, separator rows, max interface per
 * shard, this process's first shard: interior rows, interior solves (0
 * level-scheduled, 2 / 3 the 2D / 3D wavefront), separator solves (0
 * level-scheduled launches, 1 the fused separator step, 2 / 3 wavefront),
 * local vector length (slots), shards in this process, halo doubles exchanged
 * per all-gather (received, per shard) */
int gg_dd_info(gg_dd *d, int *info);
/* *on = 1 when the orthogonalization runs with its exchanges inside its
 * kernels (GG_DD_IPC / GG_DD_LOOPBACK, P > 1, environment GG_DD_XK=1 at
 * gg_dd_create; measured slower than the default), else 0 */
int gg_dd_xk_active(gg_dd *d, int *on);
/* the arrow permutation in use: pinv[j] = new index of node j; q = its inverse */
int gg_dd_perm(gg_dd *d, int *pinv, int *q);

/* the reduction order of the shard's dots (for order-matched parity checks):
 * out[slot] = permuted row of each slot of the part's dot range (-1 = padding),
 * G = block partials per shard; returns the range length (part must be held
 * by this process) */
int gg_dd_dot_layout(gg_dd *d, int part, long long *out, long long cap, int *G);

int gg_dd_solve(gg_dd *d, const double *b, double *x, const gg_options *opt, gg_result *res);
int gg_dd_solve_device(gg_dd *d, const double *d_b, double *d_x, const gg_options *opt,
                       gg_result *res);
int gg_dd_get_history(gg_dd *d, double *out, int cap);

/* Sharded BiCGStab: ggmres.h's GG_SOLVE_BICGSTAB exactly (left-preconditioned,
 * the recurrence of its description) on B with M = the sharded ILU(0) apply,
 * for the nonsymmetric systems GG_SOLVE_CG does not serve; every communicator
 * (GG_DD_LOOPBACK: timing only).  Why a second door: gg_dd_solve keeps answering
 * GG_SOLVE_BICGSTAB with GG_EINVAL (above), so the method is reached here alone.
 *   opt->flags: 0 or GG_SOLVE_BICGSTAB, both meaning BiCGStab; anything else is
 *   GG_EINVAL.  restart is validated in [1, 512] and otherwise ignored, max_iter
 *   >= 0, tol as there.  GG_ESTATE before gg_dd_set_system.
 *   An iteration is two SpMVs, two applies and three all-gathers of dot partials
 *   whatever its number: rt.v's G per shard, ONE of 2 G carrying t.s and t.t, ONE
 *   of 2 G carrying r.r and rt.r.  No basis, no Hessenberg.
 *   gg_result: iters = inner_iters = the iterations performed, restarts = 0,
 *   relres = the last ||r|| / normb; gg_dd_get_history: the initial value, then
 *   one entry per iteration.  GG_EBREAKDOWN when rt.v, omega or the next rho is
 *   zero or not finite while the solve has not converged: x then holds the last
 *   iterate on the rows this process holds, gg_last_error the text ("gg_dd_solve_
 *   bicgstab: BiCGStab broke down at iteration k: <scalar> = <value> ..."), and
 *   the object is clean for the next solve of any method.  The host enqueues the
 *   iterations in chunks as for GG_SOLVE_CG (half as long); the results do not
 *   depend on the chunk length. */
int gg_dd_solve_bicgstab(gg_dd *d, const double *b, double *x, const gg_options *opt, gg_result *res);
int gg_dd_solve_bicgstab_device(gg_dd *d, const double *d_b, double *d_x, const gg_options *opt,
                                gg_result *res);

/* The sharded backward-Euler transient loop: gg_transient_src of ggmres.h on the
 * system given to gg_dd_set_system (A = G + C/h; cdiag = C/h), over every
 * communicator (GG_DD_LOOPBACK: timing only, as for the solve).  Step it =
 * 1..nsteps solves A x_it = B u(it h) + (C/h) x_{it-1}, warm-started from
 * x_{it-1}: B the sources' incidence matrix (src_node), u their DC / PULSE / PWL
 * values (src_kind / src_ptr / src_data as gg_transient_src validates them).
 * The state stays in the shards' slots between the steps: x is gathered in once
 * before step 1 and scattered out once after the last step, the right-hand side
 * is formed on the device in slot order with the natural-order kernel's
 * operations per row (the same bits as w = B u + (C/h) x formed on the host in
 * the reference's order and passed to gg_dd_solve with x as the start), and the
 * ports are captured on the device.
 *   Arrays: host arrays, natural order, identical on every rank.  x is the
 *   initial state in, the final state out: a process writes the rows it holds,
 *   as gg_dd_solve.  port_out[j*(nsteps+1) + it], column 0 = the initial x: a
 *   process writes the rows of the ports it holds and leaves the others
 *   untouched (GG_DD_LOCAL: all of them; a separator port is held by every
 *   process); nport = 0: port and port_out may be NULL.  *iters_total = the sum
 *   of the steps' iteration counts, identical on every rank.
 *   Methods: opt->flags 0, GG_SOLVE_CGS2 or GG_SOLVE_CG, every other combination
 *   GG_EINVAL, exactly as gg_dd_solve; restart, max_iter and tol apply per step.
 *   A GG_SOLVE_CG step's first chunk of iterations is the previous step's count
 *   + 2 whenever that step returned a status >= 0 -- a count read from the
 *   replicated control block, the same on every rank; the results do not depend
 *   on it.  gg_dd_set_transient_hint(d, 0) (every rank alike) enqueues every
 *   step as gg_dd_solve does, for A/B runs; the Python binding makes that call
 *   from the environment word GG_DD_TRANSIENT_HINT=0, read at every transient
 *   call.  The GMRES steps run whole cycles.
 *   Returns GG_OK, or the status of the last step that did not return GG_OK: a
 *   step that exhausts max_iter (1) or breaks down (GG_EBREAKDOWN) does not stop
 *   the loop; after a CG breakdown x keeps the step's last iterate and the
 *   object is clean for the next step.  Every argument is checked before
 *   anything is enqueued, so every rank refuses alike: GG_EINVAL for null
 *   arguments, negative counts, a source node or port outside [0, n), a source
 *   kind or parameter length gg_transient_src refuses; GG_ESTATE before
 *   gg_dd_set_system.  gg_dd_get_history afterwards: the last step's history.
 * gg_dd_transient: the all-PULSE form (pulse[7 * k ..]: vlo, vhi, td, tr, tf, tw,
 * tp), as gg_transient is over gg_transient_src.
 * Not offered on shards: tap statistics (gg_transient_set_taps), the general MNA
 * form (gg_transient_mna) and a many-scenario batch. */
int gg_dd_transient_src(gg_dd *d, int nsteps, double h, const double *cdiag, int nsrc,
                        const int *src_node, const int *src_kind, const int *src_ptr,
                        const double *src_data, int nport, const int *port, double *x,
                        const gg_options *opt, double *port_out, int *iters_total);
int gg_dd_transient(gg_dd *d, int nsteps, double h, const double *cdiag, int nsrc,
                    const int *src_node, const double *pulse, int nport, const int *port,
                    double *x, const gg_options *opt, double *port_out, int *iters_total);
/* The same two loops with every step a gg_dd_solve_bicgstab solve: arguments,
 * outputs, checks and return value as above, opt->flags 0 or GG_SOLVE_BICGSTAB
 * (anything else GG_EINVAL).  A step's first chunk takes the hint as a CG step's
 * does; after a breakdown x keeps the step's last iterate and the loop goes on. */
int gg_dd_transient_bicgstab_src(gg_dd *d, int nsteps, double h, const double *cdiag, int nsrc,
                                 const int *src_node, const int *src_kind, const int *src_ptr,
                                 const double *src_data, int nport, const int *port, double *x,
                                 const gg_options *opt, double *port_out, int *iters_total);
int gg_dd_transient_bicgstab(gg_dd *d, int nsteps, double h, const double *cdiag, int nsrc,
                             const int *src_node, const double *pulse, int nport, const int *port,
                             double *x, const gg_options *opt, double *port_out, int *iters_total);
/* on = 0: the CG and BiCGStab steps of the following gg_dd_transient* calls take
 * no hint (default 1); set it alike on every rank */
int gg_dd_set_transient_hint(gg_dd *d, int on);

/* single operators (host vectors, natural order) for parity tests */
int gg_dd_spmv(gg_dd *d, const double *x, double *y);
int gg_dd_precond_apply(gg_dd *d, const double *in, double *out);
/* division in the shards' wavefront triangular solves (ggmres.h gg_set_division:
 * GG_DIV_FMA fuses the rows of the interiors' unskewed 2D-grid wavefronts, the
 * other wavefronts multiply as GG_DIV_RCP; the separator's solves divide) */
int gg_dd_set_division(gg_dd *d, int mode);
/* average device time (hipEvents on the solver's stream, microseconds) of one
 * all-gather of cnt doubles per shard over this communicator -- the exchange
 * every sharded operator and dot pays (cnt <= (m+1) * G of the last solve) */
int gg_dd_time_exchange(gg_dd *d, long long cnt, int reps, double *avg_us);
/* In-solve timing of the sharded solve's families per inner iteration
 * (hipEvent pairs on the solver's stream, accounted for the iterations that
 * really ran): the interior rows' + separator rows' SpMV with its halo
 * exchange, the interior L solve, the separator step (interface exchange and
 * separator solves), the interior U solve, the orthogonalization (its
 * exchanges included).  A GG_SOLVE_CG solve accounts its iterations the same
 * way: SPMV, TRSV_L, SEP and TRSV_U once per iteration, and under
 * GG_DD_PROF_ORTH -- CG orthogonalizes nothing -- its four launches with their
 * two all-gathers, as two marks per iteration: p.q partials | all-gather | x, r
 * update, and r.z, z.z partials | all-gather | p update.  A gg_dd_solve_bicgstab
 * solve: SPMV, TRSV_L, SEP and TRSV_U twice per iteration, and under
 * GG_DD_PROF_ORTH three marks, one per all-gather with the launches around it:
 * rt.v partials | all-gather | s; t.s, t.t partials | all-gather | x, r update;
 * all-gather | p update.
 * kinds: a mask of (1 << GG_DD_PROF_*). */
enum gg_dd_prof_kind {
    GG_DD_PROF_SPMV = 0, GG_DD_PROF_TRSV_L = 1, GG_DD_PROF_SEP = 2, GG_DD_PROF_TRSV_U = 3,
    GG_DD_PROF_ORTH = 4, GG_DD_PROF_NKINDS = 5
};
int gg_dd_profile_enable(gg_dd *d, int kinds);
int gg_dd_profile_reset(gg_dd *d);
int gg_dd_profile_get(gg_dd *d, int kind, int *launches, double *total_ms);
/* algorithmic bytes of one launch of family `kind`
 * (GG_DD_PROF_SPMV / _TRSV_L / _TRSV_U) over the shards of this process */
int gg_dd_bytes(gg_dd *d, int kind, double *bytes);

#ifdef __cplusplus
}
#endif
#endif
