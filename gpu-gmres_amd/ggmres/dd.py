"""Sharded GMRES(m), conjugate gradients or BiCGStab + ILU(0) over P GPUs
(include/ggmres_dd.h).

DD(nparts, device=0)                    all shards in this process on one GPU
DD(nparts, rank=r, uid=bytes, device=d) one shard per process (RCCL); uid from
                                        unique_id() on rank 0, broadcast by the caller
DD(nparts, rank=r, comm="ipc", device=d) one shard per process, device-initiated
                                        exchanges through hipIpc-mapped areas; then
                                        d.connect_ipc(allgather) with any host
                                        all-gather of bytes (e.g. torch.distributed)
DD(nparts, rank=r, comm="loopback")     timing only: shard r alone, every exchange the
                                        in-process all-gather over its own buffer (run a
                                        fixed iteration count: the values are not the system's)
"""
import ctypes
import os

import numpy as np

from . import Options, Result, _check, _csr_arrays, lib

LOCAL, RCCL, IPC, LOOPBACK = 0, 1, 2, 3
ID_BYTES = 128
IPC_HANDLE_BYTES = 64
_VP = ctypes.c_void_p
_I = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_D = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_done = False

EXPORTS = ["gg_dd_unique_id", "gg_dd_create", "gg_dd_destroy", "gg_dd_comm_ranks",
           "gg_dd_ipc_handle", "gg_dd_ipc_connect",
           "gg_dd_set_system", "gg_dd_info", "gg_dd_xk_active",
           "gg_dd_perm", "gg_dd_dot_layout", "gg_dd_solve", "gg_dd_solve_device",
           "gg_dd_transient_src", "gg_dd_transient", "gg_dd_set_transient_hint", "gg_dd_get_history", "gg_dd_spmv", "gg_dd_precond_apply", "gg_dd_set_division",
           "gg_dd_time_exchange", "gg_dd_profile_enable", "gg_dd_profile_reset", "gg_dd_profile_get",
           "gg_dd_bytes",
           "gg_dd_solve_bicgstab", "gg_dd_solve_bicgstab_device",
           "gg_dd_transient_bicgstab_src", "gg_dd_transient_bicgstab"]
# gg_dd_prof_kind (ggmres_dd.h)
PROF_SPMV, PROF_TRSV_L, PROF_SEP, PROF_TRSV_U, PROF_ORTH = range(5)
PROF_NAMES = ("spmv", "trsv_L", "separator", "trsv_U", "orthogonalization")


def _lib():
    global _done
    L = lib()
    if not _done:
        L.gg_dd_unique_id.argtypes = [ctypes.c_char_p]
        L.gg_dd_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_char_p, ctypes.POINTER(_VP)]
        L.gg_dd_destroy.argtypes = [_VP]
        L.gg_dd_ipc_handle.argtypes = [_VP, ctypes.c_char_p]
        L.gg_dd_ipc_connect.argtypes = [_VP, ctypes.c_char_p]
        L.gg_dd_comm_ranks.argtypes = [_VP, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.gg_dd_set_system.argtypes = [_VP, ctypes.c_int, _I, _I, _D, ctypes.c_int]
        L.gg_dd_info.argtypes = [_VP, _I]
        L.gg_dd_xk_active.argtypes = [_VP, ctypes.POINTER(ctypes.c_int)]
        L.gg_dd_perm.argtypes = [_VP, _I, _I]
        L.gg_dd_dot_layout.argtypes = [_VP, ctypes.c_int, _VP, ctypes.c_longlong,
                                       ctypes.POINTER(ctypes.c_int)]
        L.gg_dd_solve.argtypes = [_VP, _D, _D, ctypes.POINTER(Options), ctypes.POINTER(Result)]
        L.gg_dd_solve_device.argtypes = [_VP, _VP, _VP, ctypes.POINTER(Options),
                                         ctypes.POINTER(Result)]
        L.gg_dd_transient_src.argtypes = [_VP, ctypes.c_int, ctypes.c_double, _D, ctypes.c_int, _I, _I, _I, _D,
                                          ctypes.c_int, _VP, _D, ctypes.POINTER(Options), _VP,
                                          ctypes.POINTER(ctypes.c_int)]
        L.gg_dd_transient.argtypes = [_VP, ctypes.c_int, ctypes.c_double, _D, ctypes.c_int, _I, _D,
                                      ctypes.c_int, _VP, _D, ctypes.POINTER(Options), _VP,
                                      ctypes.POINTER(ctypes.c_int)]
        L.gg_dd_solve_bicgstab.argtypes = L.gg_dd_solve.argtypes
        L.gg_dd_solve_bicgstab_device.argtypes = L.gg_dd_solve_device.argtypes
        L.gg_dd_transient_bicgstab_src.argtypes = L.gg_dd_transient_src.argtypes
        L.gg_dd_transient_bicgstab.argtypes = L.gg_dd_transient.argtypes
        L.gg_dd_set_transient_hint.argtypes = [_VP, ctypes.c_int]
        L.gg_dd_get_history.argtypes = [_VP, _VP, ctypes.c_int]
        L.gg_dd_spmv.argtypes = [_VP, _D, _D]
        L.gg_dd_precond_apply.argtypes = [_VP, _D, _D]
        L.gg_dd_set_division.argtypes = [_VP, ctypes.c_int]
        L.gg_dd_time_exchange.argtypes = [_VP, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        L.gg_dd_profile_enable.argtypes = [_VP, ctypes.c_int]
        L.gg_dd_profile_reset.argtypes = [_VP]
        L.gg_dd_profile_get.argtypes = [_VP, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(ctypes.c_double)]
        L.gg_dd_bytes.argtypes = [_VP, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        _done = True
    return L


def unique_id():
    buf = ctypes.create_string_buffer(ID_BYTES)
    _check(_lib().gg_dd_unique_id(buf))
    return buf.raw


class DD:
    def __init__(self, nparts, device=0, rank=None, uid=None, comm=None):
        h = _VP()
        kind = IPC if comm == "ipc" else LOOPBACK if comm == "loopback" else LOCAL if rank is None else RCCL
        if kind in (IPC, LOOPBACK) and rank is None:
            raise ValueError(f"dd: comm={comm!r} needs a rank")
        _check(_lib().gg_dd_create(int(device), int(nparts), kind, int(rank or 0),
                                   uid if uid is not None else None, ctypes.byref(h)))
        self.h, self.P, self.kind, self.rank = h, nparts, kind, rank
        self.n = 0

    def ipc_handle(self):
        """this rank's exchange-area handle (GG_DD_IPC)"""
        buf = ctypes.create_string_buffer(IPC_HANDLE_BYTES)
        _check(_lib().gg_dd_ipc_handle(self.h, buf))
        return buf.raw

    def ipc_connect(self, handles):
        """every rank's handle, rank order: maps the peers' areas (collective)"""
        if len(handles) != self.P or any(len(x) != IPC_HANDLE_BYTES for x in handles):
            raise ValueError("dd: need nparts handles of IPC_HANDLE_BYTES")
        _check(_lib().gg_dd_ipc_connect(self.h, b"".join(handles)))

    def connect_ipc(self, allgather):
        """allgather(bytes) -> list of every rank's bytes (rank order)"""
        self.ipc_connect(list(allgather(self.ipc_handle())))

    def close(self):
        if self.h:
            _lib().gg_dd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def comm_ranks(self):
        """(ranks in the exchange, this process's rank): RCCL ncclCommCount, IPC the
        mapped areas (collective: every rank must call it), LOCAL (1, 0)"""
        c, r = ctypes.c_int(), ctypes.c_int()
        _check(_lib().gg_dd_comm_ranks(self.h, ctypes.byref(c), ctypes.byref(r)))
        return c.value, r.value

    def set_system(self, A, method=1):
        n, rp, ci, v = _csr_arrays(A)
        self.n = n
        _check(_lib().gg_dd_set_system(self.h, n, rp, ci, v, int(method)))

    def info(self):
        a = np.zeros(10, np.int32)
        _check(_lib().gg_dd_info(self.h, a))
        keys = ["n", "nparts", "nsep", "max_iface", "n_interior", "wave_interior", "wave_separator",
                "local_len", "shards_here", "halo_doubles"]
        out = dict(zip(keys, (int(x) for x in a)))
        on = ctypes.c_int()
        _check(_lib().gg_dd_xk_active(self.h, ctypes.byref(on)))
        out["cgs2_in_kernel_exchange"] = on.value
        return out

    def perm(self):
        pinv = np.zeros(self.n, np.int32)
        q = np.zeros(self.n, np.int32)
        _check(_lib().gg_dd_perm(self.h, pinv, q))
        return pinv, q

    def dot_layout(self, part):
        G = ctypes.c_int()
        ln = _check(_lib().gg_dd_dot_layout(self.h, int(part), None, 0, ctypes.byref(G)), True)
        out = np.zeros(max(ln, 1), np.int64)
        _lib().gg_dd_dot_layout(self.h, int(part), out.ctypes.data, ln, ctypes.byref(G))
        return out[:ln], G.value

    def solve(self, b, x0=None, restart=30, max_iter=3000, tol=1e-10, flags=0):
        """flags: ggmres.SOLVE_CGS2 for the three-all-gather orthogonalization, or
        ggmres.SOLVE_CG for conjugate gradients (B and its ILU(0) SPD): ret is then
        0, 1 or ggmres.EBREAKDOWN -- returned, not raised, with x the last iterate,
        the history and the counts, as ggmres.Solver.solve does"""
        return self._solve(_lib().gg_dd_solve, b, x0, restart, max_iter, tol, flags)

    def _solve(self, fn, b, x0, restart, max_iter, tol, flags):
        b = np.ascontiguousarray(b, np.float64)
        x = np.zeros(self.n) if x0 is None else np.array(x0, np.float64, copy=True)
        o = Options(int(restart), int(max_iter), float(tol), int(flags))
        r = Result()
        rc = _check(fn(self.h, b, x, ctypes.byref(o), ctypes.byref(r)), allow_nc=True)
        return dict(ret=rc, x=x, iters=r.iters, inner=r.inner_iters, restarts=r.restarts,
                    relres=r.relres, solve_ms=r.solve_ms, hist=self.history())

    def solve_device(self, b_ptr, x_ptr, restart=30, max_iter=3000, tol=1e-10, flags=0):
        return self._solve_device(_lib().gg_dd_solve_device, b_ptr, x_ptr, restart, max_iter, tol, flags)

    def _solve_device(self, fn, b_ptr, x_ptr, restart, max_iter, tol, flags):
        o = Options(int(restart), int(max_iter), float(tol), int(flags))
        r = Result()
        rc = _check(fn(self.h, _VP(b_ptr), _VP(x_ptr), ctypes.byref(o), ctypes.byref(r)), allow_nc=True)
        return dict(ret=rc, iters=r.iters, inner=r.inner_iters, restarts=r.restarts,
                    relres=r.relres, solve_ms=r.solve_ms)

    def solve_bicgstab(self, b, x0=None, restart=30, max_iter=3000, tol=1e-10, flags=0):
        """gg_dd_solve_bicgstab: BiCGStab on the shards (flags 0 or ggmres.SOLVE_BICGSTAB,
        both BiCGStab -- DD.solve refuses that flag); the dict of solve, ret 0, 1 or
        ggmres.EBREAKDOWN (returned, not raised, with x the last iterate)"""
        return self._solve(_lib().gg_dd_solve_bicgstab, b, x0, restart, max_iter, tol, flags)

    def solve_bicgstab_device(self, b_ptr, x_ptr, restart=30, max_iter=3000, tol=1e-10, flags=0):
        return self._solve_device(_lib().gg_dd_solve_bicgstab_device, b_ptr, x_ptr, restart, max_iter, tol,
                                  flags)

    def _transient_io(self, nsteps, ports, x0, x_fill, port_fill):
        """the in/out state, the port array (preset to port_fill) and the rows of x
        this process writes back (x_fill given: asked of gg_dd_spmv, which writes
        the same rows -- x itself is the C entry point's input, so it cannot be preset)"""
        # the hint's switch, read at every call: GG_DD_TRANSIENT_HINT=0 turns it off
        off = os.environ.get("GG_DD_TRANSIENT_HINT", "")[:1] == "0"
        _check(_lib().gg_dd_set_transient_hint(self.h, 0 if off else 1))
        x = np.array(x0, np.float64, copy=True)
        ports = np.ascontiguousarray(ports, np.int32)
        pv = np.full(max(len(ports), 1) * (nsteps + 1), 0.0 if port_fill is None else float(port_fill))
        own = None
        if x_fill is not None:
            own = ~np.isnan(self.spmv(np.zeros(self.n), np.full(self.n, np.nan)))
        return x, ports, pv, own

    def _transient_out(self, rc, nsteps, ports, x, pv, own, x_fill, tot):
        if own is not None:
            x = np.where(own, x, float(x_fill))
        return dict(ret=rc, x=x, ports=pv[: len(ports) * (nsteps + 1)].reshape(len(ports), nsteps + 1),
                    iters_total=tot.value)

    def transient_src(self, nsteps, h, cdiag, src_node, sources, ports, x0, restart=32, max_iter=10000,
                      tol=1e-7, flags=0, x_fill=None, port_fill=None):
        """gg_dd_transient_src: the backward-Euler loop over the shards, the state in
        their slots between the steps; sources = [(kind, params), ...] (ggmres.SRC_DC
        / SRC_PULSE / SRC_PWL), flags 0, ggmres.SOLVE_CGS2 or ggmres.SOLVE_CG.
        Returns dict(ret, x, ports [nport, nsteps+1], iters_total); ret is GG_OK or
        the status of the last step that was not (1, ggmres.EBREAKDOWN: returned,
        not raised).  port_fill presets the port array and x_fill stands in the
        rows of x this process does not hold (e.g. NaN), so a rank sees what it wrote.
        Environment GG_DD_TRANSIENT_HINT=0, read at every call (set it alike on every
        rank): the CG steps take no hint (gg_dd_set_transient_hint)."""
        return self._transient_src(_lib().gg_dd_transient_src, nsteps, h, cdiag, src_node, sources, ports, x0,
                                   restart, max_iter, tol, flags, x_fill, port_fill)

    def transient_bicgstab_src(self, nsteps, h, cdiag, src_node, sources, ports, x0, restart=32, max_iter=10000,
                               tol=1e-7, flags=0, x_fill=None, port_fill=None):
        """gg_dd_transient_bicgstab_src: transient_src with every step a BiCGStab solve
        (flags 0 or ggmres.SOLVE_BICGSTAB); the steps take the hint as CG's do"""
        return self._transient_src(_lib().gg_dd_transient_bicgstab_src, nsteps, h, cdiag, src_node, sources,
                                   ports, x0, restart, max_iter, tol, flags, x_fill, port_fill)

    def _transient_src(self, fn, nsteps, h, cdiag, src_node, sources, ports, x0, restart, max_iter, tol, flags,
                       x_fill, port_fill):
        x, ports, pv, own = self._transient_io(nsteps, ports, x0, x_fill, port_fill)
        src_node = np.ascontiguousarray(src_node, np.int32)
        kind = np.array([k for k, _ in sources], np.int32)
        ptr = np.zeros(len(sources) + 1, np.int32)
        ptr[1:] = np.cumsum([len(q) for _, q in sources])
        data = np.concatenate([np.asarray(q, np.float64) for _, q in sources]) if sources else np.zeros(1)
        tot = ctypes.c_int()
        o = Options(int(restart), int(max_iter), float(tol), int(flags))
        one = np.zeros(1, np.int32)
        rc = _check(fn(
            self.h, int(nsteps), float(h), np.ascontiguousarray(cdiag, np.float64), len(src_node),
            src_node if len(src_node) else one, kind if len(kind) else one, ptr, data, len(ports),
            ports.ctypes.data if len(ports) else None, x, ctypes.byref(o),
            pv.ctypes.data if len(ports) else None, ctypes.byref(tot)), allow_nc=True)
        return self._transient_out(rc, nsteps, ports, x, pv, own, x_fill, tot)

    def transient(self, nsteps, h, cdiag, src_node, pulse, ports, x0, restart=32, max_iter=10000,
                  tol=1e-7, flags=0, x_fill=None, port_fill=None):
        """gg_dd_transient: transient_src with PULSE rows pulse[nsrc, 7]"""
        return self._transient(_lib().gg_dd_transient, nsteps, h, cdiag, src_node, pulse, ports, x0, restart,
                               max_iter, tol, flags, x_fill, port_fill)

    def transient_bicgstab(self, nsteps, h, cdiag, src_node, pulse, ports, x0, restart=32, max_iter=10000,
                           tol=1e-7, flags=0, x_fill=None, port_fill=None):
        """gg_dd_transient_bicgstab: transient_bicgstab_src with PULSE rows pulse[nsrc, 7]"""
        return self._transient(_lib().gg_dd_transient_bicgstab, nsteps, h, cdiag, src_node, pulse, ports, x0,
                               restart, max_iter, tol, flags, x_fill, port_fill)

    def _transient(self, fn, nsteps, h, cdiag, src_node, pulse, ports, x0, restart, max_iter, tol, flags,
                   x_fill, port_fill):
        x, ports, pv, own = self._transient_io(nsteps, ports, x0, x_fill, port_fill)
        src_node = np.ascontiguousarray(src_node, np.int32)
        pulse = np.ascontiguousarray(pulse, np.float64).reshape(-1)
        tot = ctypes.c_int()
        o = Options(int(restart), int(max_iter), float(tol), int(flags))
        rc = _check(fn(
            self.h, int(nsteps), float(h), np.ascontiguousarray(cdiag, np.float64), len(src_node),
            src_node if len(src_node) else np.zeros(1, np.int32), pulse if pulse.size else np.zeros(7),
            len(ports), ports.ctypes.data if len(ports) else None, x, ctypes.byref(o),
            pv.ctypes.data if len(ports) else None, ctypes.byref(tot)), allow_nc=True)
        return self._transient_out(rc, nsteps, ports, x, pv, own, x_fill, tot)

    def history(self):
        n = _lib().gg_dd_get_history(self.h, None, 0)
        out = np.zeros(max(n, 1))
        _lib().gg_dd_get_history(self.h, out.ctypes.data, n)
        return out[:n]

    def spmv(self, x, y=None):
        y = np.zeros(self.n) if y is None else np.array(y, np.float64, copy=True)
        _check(_lib().gg_dd_spmv(self.h, np.ascontiguousarray(x, np.float64), y))
        return y

    def set_division(self, mode):
        """ggmres.DIV_EXACT / DIV_RCP / DIV_FMA for the shards' wavefront triangular solves"""
        _check(_lib().gg_dd_set_division(self.h, int(mode)))

    def profile(self, on=True, kinds=None):
        """in-solve timing of the families (PROF_*) of every inner iteration"""
        mask = 0
        if on:
            mask = (1 << len(PROF_NAMES)) - 1 if kinds is None else sum(1 << k for k in kinds)
        _check(_lib().gg_dd_profile_reset(self.h))
        _check(_lib().gg_dd_profile_enable(self.h, mask))

    def profile_get(self, kind):
        n, ms = ctypes.c_int(), ctypes.c_double()
        _check(_lib().gg_dd_profile_get(self.h, int(kind), ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def bytes(self, kind):
        """algorithmic bytes of one launch of family kind (PROF_SPMV / _TRSV_L / _TRSV_U), this process's shards"""
        b = ctypes.c_double()
        _check(_lib().gg_dd_bytes(self.h, int(kind), ctypes.byref(b)))
        return b.value

    def time_exchange(self, cnt, reps=200):
        """average microseconds of one all-gather of cnt doubles per shard"""
        us = ctypes.c_double()
        _check(_lib().gg_dd_time_exchange(self.h, int(cnt), int(reps), ctypes.byref(us)))
        return us.value

    def precond_apply(self, v, out=None):
        out = np.zeros(self.n) if out is None else np.array(out, np.float64, copy=True)
        _check(_lib().gg_dd_precond_apply(self.h, np.ascontiguousarray(v, np.float64), out))
        return out
