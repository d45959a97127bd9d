"""Every getenv("GG_...") switch under gpu-gmres_amd/csrc is accounted for: it
maps either to the test that runs its other position(s) or to the reason it
needs none.  A switch added later fails here until it has an entry (and
DESIGN.md "9. Switches" carries the same table, with the defaults)."""
import glob
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gpu-gmres_amd", "csrc")

V = "tests/test_gpu_variants.py"
# name -> ("test", file, what in it names the switch) | ("exempt", reason)
SWITCHES = {
    # ---- launch forms compared with the default child's bits (test_gpu_variants.py)
    "GG_MGS_GATHER": ("test", V, "cases A, A1, E"),
    "GG_MGS_PREFETCH": ("test", V, "cases A, A1, E"),
    "GG_CYCLE_PIPE": ("test", V, "cases A, A1, Apad"),
    "GG_NO_PADSKIP": ("test", V, "cases A, A1, Apad, Epad"),
    "GG_NO_PERSIST": ("test", V, "cases A, A1"),
    "GG_NO_WAVEFRONT": ("test", V, "cases A1, Bbpc"),
    "GG_FLOW_LONG": ("test", V, "cases B, Bbpc"),
    "GG_FLOW_BPC": ("test", V, "case Bbpc"),
    "GG_FLOW_FILLFOLD": ("test", V, "case C"),
    "GG_SPLIT_DIVFOLD": ("test", V, "case Cf"),
    "GG_SPLIT_MULFOLD": ("test", V, "cases C, Cf"),
    "GG_SPMV_XDIV": ("test", V, "case C"),
    "GG_TAIL_SMALL": ("test", V, "case D"),
    "GG_BATCH_MGS": ("test", V, "cases E, Efix, F"),
    "GG_BATCH_MGS2": ("test", V, "cases E, Efix"),
    "GG_BATCH_CHUNK": ("test", V, "cases E, Efix, F"),
    "GG_BATCH_ZMAP": ("test", V, "cases E, Efix"),
    "GG_BATCH_S1_SINGLE": ("test", V, "cases E, Efix"),
    "GG_TRANSIENT_HINT": ("test", V, "case F"),
    "GG_CG_BATCH_CHUNK": ("test", V, "case G"),
    "GG_FMA_TILE": ("test", V, "test_fma_tile_mix"),
    "GG_WAVE3D_PLANES": ("test", V, "test_grid3d_other_layouts"),
    "GG_NO_WAVE3D": ("test", V, "test_grid3d_other_layouts"),
    # ---- read at every use: flipped inside the pytest process by other modules
    "GG_BATCH_SEQ": ("test", "tests/test_gpu_batch.py", "test_solve_batch_sequential_fallback"),
    "GG_DD_HALO_FUSED": ("test", "tests/test_gpu_dd_modes.py", "GG_DD_HALO_FUSED"),
    "GG_DD_HALO_INLINE": ("test", "tests/test_gpu_dd_modes.py", "GG_DD_HALO_INLINE"),
    "GG_DD_SEPFLOW": ("test", "tests/test_gpu_dd.py", "GG_DD_SEPFLOW"),
    "GG_DD_XK": ("test", "tests/test_gpu_dd_ranks.py", "GG_DD_XK"),
    "GG_FLOW_ELL": ("test", "tests/test_gpu_parity.py", "test_gmres_split_parity"),
    "GG_FLOW_RCM": ("test", "tests/test_gpu_parity.py", "test_gmres_split_parity_natural_layout"),
    "GG_FMA_SKEW": ("test", "tests/test_gpu_fastdiv.py", "test_fma_fallbacks"),
    "GG_FUSE_SPMV": ("test", "tests/test_gpu_fastdiv.py", "GG_FUSE_SPMV"),
    "GG_ILUK_LONG": ("test", "tests/test_gpu_parity.py", "test_iluk_device_factors_bitexact"),
    "GG_ILUK_SERIAL": ("test", "tests/test_switch_table.py", "test_iluk_serial_pattern"),
    "GG_NO_BORDER": ("test", "tests/test_gpu_border.py", "test_no_border_flow_kernel_same_bits"),
    "GG_PERSIST_TEST_LDS": ("test", "tests/test_gpu_residency.py", "GG_PERSIST_TEST_LDS"),
    "GG_SPMV_CSR": ("test", "tests/test_gpu_ainv.py", "GG_SPMV_CSR"),
    "GG_SPMV_PANEL": ("test", "tests/test_gpu_parity.py", "test_spmv_panels_bitexact"),
    "GG_SPMV_PANEL_MIN": ("test", "tests/test_gpu_parity.py", "test_spmv_panels_bitexact"),
    "GG_SPMV_RTILE": ("test", "tests/test_gpu_parity.py", "test_spmv_panels_bitexact"),
    "GG_TILE_GRID": ("test", "tests/test_gpu_residency.py", "GG_TILE_GRID"),
    "GG_TILE_QUEUE": ("test", "tests/test_gpu_residency.py", "GG_TILE_QUEUE"),
    "GG_TRSV_LEVELS": ("test", "tests/test_gpu_parity.py", "test_ilu0_apply_bitexact"),
    "GG_WAVE_HWDIV": ("test", "tests/test_gpu_parity.py", "test_wavefront_division_modes"),
    "GG_WIDE_FORCE": ("test", "tests/test_gpu_parity.py", "test_gmres_wide_orthogonalization_parity"),
    # ---- no launch form behind them
    "GG_MGS_TRACE": ("exempt", "diagnostic trace: time stamps of one launch to stderr, the same kernel and arguments"),
    "GG_HOST_THREADS": ("exempt", "host thread count of the setup phase (tests/test_abi.py runs 1 and 4 threads)"),
    "GG_DD_IPC_CAP": ("exempt", "size of the IPC exchange area in doubles, no other kernel or launch"),
}


def switches_in_source():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "**", "*"), recursive=True):
        if os.path.isfile(path):
            with open(path, errors="replace") as f:
                names |= set(re.findall(r'getenv\(\s*"(GG_[A-Z0-9_]+)"', f.read()))
    return names


def test_every_switch_is_covered_or_exempt():
    found = switches_in_source()
    assert len(found) >= 40                       # the scan reads the sources
    assert not found - set(SWITCHES), f"switches without a test or an exemption: {sorted(found - set(SWITCHES))}"
    assert not set(SWITCHES) - found, f"entries for switches the sources no longer read: {sorted(set(SWITCHES) - found)}"
    for name, entry in SWITCHES.items():
        if entry[0] == "exempt":
            assert len(entry) == 2 and entry[1].strip() and "\n" not in entry[1], name
            continue
        kind, path, what = entry
        assert kind == "test"
        with open(os.path.join(REPO, path)) as f:
            text = f.read()
        assert name in text, f"{path} does not name {name}"
        if not what.startswith("case"):
            assert what in text, f"{path}: no {what}"


def test_variant_cases_name_their_switches():
    """the table's "case X" entries against test_gpu_variants' own tables"""
    import test_gpu_variants as T
    for name, entry in SWITCHES.items():
        if entry[0] != "test" or entry[1] != V or not entry[2].startswith("case"):
            continue
        for case in re.sub(r"^cases? ", "", entry[2]).replace("'s environment", "").split(", "):
            base, variants = T.CASES[case]
            assert name in base or any(name in env for env in variants.values()), (name, case)


def test_design_md_lists_every_switch():
    with open(os.path.join(REPO, "DESIGN.md")) as f:
        text = f.read()
    table = text[re.search(r"^## .*Switches", text, re.M).start():]
    for name in SWITCHES:
        assert f"`{name}`" in table, name


@pytest.mark.parametrize("case", ["9pt_10x10.mtx", "rand300"])
def test_iluk_serial_pattern(ggmres_lib, case, monkeypatch):
    """GG_ILUK_SERIAL=1 (levels >= 2: lofC itself instead of the row-parallel
    fill paths): the same pattern, which test_abi.py pins to the oracle's"""
    from test_abi import host_iluk_pattern, load, random_nonsym
    A = random_nonsym(300, 4, 11) if case == "rand300" else load(case)
    for k in (2, 3):
        want = host_iluk_pattern(ggmres_lib, A, k, 4)
        monkeypatch.setenv("GG_ILUK_SERIAL", "1")
        got = host_iluk_pattern(ggmres_lib, A, k, 4)
        monkeypatch.delenv("GG_ILUK_SERIAL")
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (case, k)


@pytest.mark.parametrize("gather,prefetch,J,want", [
    ("2", "1", 4, "k_arnoldi_persist<4, 2, 1>"), ("0", "0", 1, "k_arnoldi_persist<1, 0, 0>"),
    ("2", "2", 4, "k_arnoldi_persist<4, 2, 2>"), ("3", "1", 2, "k_arnoldi_persist<2, 3, 1>"),
    # the settings the launch remaps: the reducer-only blocks exist with a prefetch only,
    # prefetch 2 with the elected gather only and up to 4 units per thread
    ("3", "0", 4, "k_arnoldi_persist<4, 2, 0>"), ("0", "2", 4, "k_arnoldi_persist<4, 0, 1>"),
    ("2", "2", 8, "k_arnoldi_persist<8, 2, 1>"), ("3", "2", 8, "k_arnoldi_persist<8, 3, 1>")])
def test_mgs_kernel_names_the_instantiation_launched(ggmres_lib, monkeypatch, gather, prefetch, J, want):
    """gg_mgs_kernel's name comes from the launch's own mapping (kernels/arnoldi_persist.hip
    persist_form), not from the environment's numbers -- host code, so J = 8,
    whose grid is not co-resident on an MI355X, is pinned here"""
    import ggmres
    monkeypatch.setenv("GG_MGS_GATHER", gather)
    monkeypatch.setenv("GG_MGS_PREFETCH", prefetch)
    assert ggmres.mgs_kernel_for(J) == want
