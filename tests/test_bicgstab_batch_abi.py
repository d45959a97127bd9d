"""The BiCGStab batch's entry points (include/ggmres.h,
csrc/bicgstab_batch.hip): declared in the header, exported by the built
library, resolvable through ctypes.  CPU only -- nothing is called."""
import os
import re
import subprocess

from conftest import PKG, REPO

SYMBOLS = ["gg_solve_bicgstab_batch_device", "gg_solve_bicgstab_batch", "gg_transient_bicgstab_batch"]


def declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(gg_\w+)\s*\(", txt))


def exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libggmres.so")],
                                  text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_bicgstab_batch_symbols_declared_and_exported(ggmres_lib):
    names = declared("ggmres.h")
    syms = exported()
    import ggmres
    for name in SYMBOLS:
        assert name in names, f"{name}: not declared in include/ggmres.h"
        assert name in syms, f"{name}: not exported by libggmres.so"
        assert name in ggmres.EXPORTS
        getattr(ggmres_lib, name)       # resolvable through ctypes


def test_bicgstab_batch_argument_lists_are_the_batch_ones(ggmres_lib):
    """gg_transient_bicgstab_batch takes exactly gg_transient_batch's parameter
    list, the two solves gg_solve_batch*'s: in the header and in the binding"""
    txt = open(os.path.join(REPO, "include", "ggmres.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)

    def params(name):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1)).strip()
    assert params("gg_transient_bicgstab_batch") == params("gg_transient_batch")
    assert params("gg_solve_bicgstab_batch_device") == params("gg_solve_batch_device")
    assert params("gg_solve_bicgstab_batch") == params("gg_solve_batch")
    L = ggmres_lib
    assert L.gg_transient_bicgstab_batch.argtypes == L.gg_transient_batch.argtypes
    assert L.gg_solve_bicgstab_batch_device.argtypes == L.gg_solve_batch_device.argtypes
    assert L.gg_solve_bicgstab_batch.argtypes == L.gg_solve_batch.argtypes


def test_python_binding_has_the_three_methods():
    import ggmres
    for name in ("solve_bicgstab_batch", "solve_bicgstab_batch_device", "transient_bicgstab_batch"):
        assert callable(getattr(ggmres.Solver, name)), name
