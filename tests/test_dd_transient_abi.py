"""The sharded transient loop's entry points (include/ggmres_dd.h, csrc/dd.hip):
declared in the header, exported by the built library, listed in
ggmres.dd.EXPORTS and resolvable through ctypes.  CPU only -- nothing is called."""
import os
import re
import subprocess

from conftest import PKG, REPO

SYMBOLS = ["gg_dd_transient_src", "gg_dd_transient", "gg_dd_set_transient_hint"]


def header(name):
    txt = open(os.path.join(REPO, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def params(txt, name):
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m, name
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_dd_transient_symbols_declared_exported_and_listed(ggmres_lib):
    names = set(re.findall(r"\b(gg_\w+)\s*\(", header("ggmres_dd.h")))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libggmres.so")],
                                  text=True)
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from ggmres import dd
    for name in SYMBOLS:
        assert name in names, f"{name}: not declared in include/ggmres_dd.h"
        assert name in syms, f"{name}: not exported by libggmres.so"
        assert name in dd.EXPORTS
        getattr(ggmres_lib, name)       # resolvable through ctypes


def test_dd_transient_argument_lists_follow_the_single_device_loops():
    """gg_dd_transient_src / gg_dd_transient take gg_transient_src's / gg_transient's
    parameter lists behind the object"""
    dd, one = header("ggmres_dd.h"), header("ggmres.h")
    for a, b in (("gg_dd_transient_src", "gg_transient_src"), ("gg_dd_transient", "gg_transient")):
        pa, pb = params(dd, a), params(one, b)
        assert pa[0] == "gg_dd *d" and pb[0] == "gg_solver *s"
        assert pa[1:] == pb[1:], (a, b)
