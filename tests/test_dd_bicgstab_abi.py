"""The sharded BiCGStab entry points (include/ggmres_dd.h, csrc/dd.hip): declared in
the header with the signatures of the entry points they stand beside, exported by
the built library, listed in ggmres.dd.EXPORTS and resolvable through ctypes.
CPU only -- nothing is called."""
import os
import subprocess

from conftest import PKG
from test_dd_transient_abi import header, params

PAIRS = [("gg_dd_solve_bicgstab", "gg_dd_solve"), ("gg_dd_solve_bicgstab_device", "gg_dd_solve_device"),
         ("gg_dd_transient_bicgstab_src", "gg_dd_transient_src"), ("gg_dd_transient_bicgstab", "gg_dd_transient")]


def test_dd_bicgstab_symbols_declared_exported_and_listed(ggmres_lib):
    import re
    names = set(re.findall(r"\b(gg_\w+)\s*\(", header("ggmres_dd.h")))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libggmres.so")],
                                  text=True)
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from ggmres import dd
    for name, _ in PAIRS:
        assert name in names, f"{name}: not declared in include/ggmres_dd.h"
        assert name in syms, f"{name}: not exported by libggmres.so"
        assert name in dd.EXPORTS
        getattr(ggmres_lib, name)       # resolvable through ctypes


def test_dd_bicgstab_argument_lists_are_those_of_the_existing_entry_points():
    txt = header("ggmres_dd.h")
    for new, old in PAIRS:
        assert params(txt, new) == params(txt, old), (new, old)
    assert params(txt, "gg_dd_solve_bicgstab") == [
        "gg_dd *d", "const double *b", "double *x", "const gg_options *opt", "gg_result *res"]
    assert params(txt, "gg_dd_solve_bicgstab_device") == [
        "gg_dd *d", "const double *d_b", "double *d_x", "const gg_options *opt", "gg_result *res"]


def test_dd_bicgstab_bindings_exist():
    from ggmres.dd import DD
    for name in ("solve_bicgstab", "solve_bicgstab_device", "transient_bicgstab_src", "transient_bicgstab"):
        assert callable(getattr(DD, name))
