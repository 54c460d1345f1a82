"""plaid.roast over several devices: what can be checked without a GPU -- the C ABI declarations and the header's words, the
R shim and wrappers (R is not installed: statically and with a C compiler against stand-in R headers), the Python exports,
and the device list's own checks.  (The numpy restatement's deviation from the 50-digit form, which the GPU
test's allowance is taken from, is re-measured in tests/test_roast_ref.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import roast_ref as rr
from tests.test_multi_plaid_test_host import ROOT, _args, _read

R_ARGS = 11   # R_plaidhip_roast (.Call routine)

ENTRIES = {   # the entry -> its C arguments
    "plaidhip_roast": 21, "plaidhip_roast_multi": 22, "plaidhip_dev_roast_rotate": 16, "plaidhip_dev_roast_stats": 11,
    "plaidhip_roast_rotations": 8, "plaidhip_roast_finish": 11,
}


def test_header_and_signatures_declare_the_entries():
    from plaid_amd import _lib
    header = _read("include", "plaidhip.h")
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        assert f"int {name}(" in header
        assert len(_args(header, f"int {name}")) == nargs, name
        assert len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name)
    for hookname in ("plaidhip_debug_roast_sharded_on_one_device", "plaidhip_debug_roast_normals"):
        assert hookname not in header and hasattr(lib, hookname)       # test hooks, not API
    words = header[header.index("plaid.roast(X, design, G, contrasts)"):header.index("int plaidhip_roast(")]
    for word in ("AS RECALLED", "Philox4x32-10", "Box-Muller", "mean50", "floormean", "msq", "0.67448975019608171",
                 "min(df0 + d, 10,000)", "(b + 1) / (nrot + 1)", "midp", "a stated deviation", "romer", "weights", "trend.var",
                 "dgCMatrix", 'na = "fit"', "PLAIDHIP_ROAST_MEAN50_MAX 16384", "no cap on the samples"):
        assert word in words, word
    # the blocks of plaid.fry and plaid.camera keep their words
    fry = header[header.index("plaid.fry(X, design, G, contrasts)"):header.index("int plaidhip_fry(")]
    assert "roast and mroast" in fry
    camera = header[header.index("plaid.camera(X, design, G, contrasts)"):header.index("int plaidhip_camera(")]
    assert "fry / roast" in camera


def test_shim_defines_registers_and_calls_the_entries():
    csrc = _read("r-pkg", "src", "plaidhip_R.c")
    routine = "R_plaidhip_roast"
    params = _args(csrc, "SEXP " + routine)
    assert len(params) == R_ARGS and all(p.startswith("SEXP ") for p in params)
    m = re.search(r'\{"' + routine + r'",\s*\(DL_FUNC\)&' + routine + r",\s*(\d+)\}", csrc)
    assert m and int(m.group(1)) == R_ARGS, "registration"
    body = csrc[csrc.index("SEXP " + routine + "("):]
    body = body[:body.index("\n}\n")]
    assert len(_args(body, "rc = plaidhip_roast_multi")) == ENTRIES["plaidhip_roast_multi"]
    assert len(_args(body, "rc = plaidhip_roast")) == ENTRIES["plaidhip_roast"]
    rsrc = _read("r-pkg", "R", "plaid-hip.R")
    call = [a for a in _args(rsrc[rsrc.index(f'.Call("{routine}"'):], ".Call") if not a.startswith("PACKAGE")]
    assert len(call) - 1 == R_ARGS, "the .Call passes what the routine takes"
    assert rsrc.count(f'.Call("{routine}"') == 1
    namespace = _read("r-pkg", "NAMESPACE")
    for fn in ("plaid.roast", "plaid.roast.contrasts"):
        assert re.search(r"\b" + re.escape(fn) + r"\b", namespace), fn
        assert f"\n{fn} <- function(" in rsrc, fn
        sig = rsrc[rsrc.index(f"\n{fn} <- function("):]
        sig = sig[:sig.index("{")]
        for word in ('set.statistic = "mean50"', "nrot = 1999", "seed = 1", 'zscore = "hill"', "midp = TRUE", "rotations = NULL",
                     'sort.by = "directional"'):
            assert word in sig, (fn, word)
    # the R side's option lists are the library's, in the library's order
    from plaid_amd import engine
    for name, table in ((".roast_statistics", engine.ROAST_STATISTIC), (".roast_zscores", engine.ROAST_ZSCORE)):
        listed = re.search(re.escape(name) + r" <- c\(([^)]*)\)", rsrc).group(1)
        assert [w.strip().strip('"') for w in listed.split(",")] == sorted(table, key=table.get), name


def test_r_shim_still_compiles():
    out = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                          "-I" + os.path.join(ROOT, "tests", "r_api_stub"), "-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "r-pkg", "src", "plaidhip_R.c")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_the_constants_agree():
    from plaid_amd import engine
    header = _read("include", "plaidhip.h")
    assert f"#define PLAIDHIP_ROAST_MEAN50_MAX {engine.ROAST_MEAN50_MAX}" in header
    assert engine.ROAST_MEAN50_MAX >= 4096                             # replaid.plage's cap
    assert (engine.ROAST_MEAN50_MAX + 1 + 384) * 8 <= 160 * 1024       # one rotation at an odd stride and the 3 KiB beside it
    import scipy.stats as st
    assert abs(rr.SQRT_Q - st.norm.ppf(0.75)) <= 2 ** -52             # sqrt(qchisq(0.5, 1)) = qnorm(0.75)
    assert abs(rr.SQRT_Q - np.sqrt(st.chi2.ppf(0.5, 1))) <= 1e-14       # (scipy's chi2.ppf itself is this far off)
    roast_h = _read("plaid_amd", "csrc", "roast.h")
    assert "0.67448975019608171" in roast_h


def test_python_exports():
    import plaid_amd
    for name in ("plaid_roast", "plaid_roast_contrasts", "roast_multi"):
        assert name in plaid_amd.__all__ and callable(getattr(plaid_amd, name))
    assert callable(plaid_amd.Context.roast)


def test_the_device_list_is_checked_before_anything_else():
    import plaid_amd
    from plaid_amd import engine
    rng = np.random.default_rng(1)
    X = rng.normal(size=(8, 10))
    D = rr.make_design(10, 2, rng)
    with pytest.raises(plaid_amd.PlaidHipError, match="twice"):
        engine.roast_multi(X, D, [0, 2], [0, 1], devices=[0, 1, 0])
    with pytest.raises(plaid_amd.PlaidHipError, match="ndev"):
        engine.roast_multi(X, D, [0, 2], [0, 1], devices=[])
    with pytest.raises(ValueError):
        engine.roast_multi(X, D, [0, 2], [0, 1], devices=None)


def test_hill_lies_this_far_from_the_exact_transform():
    """Hill's form against qnorm(pt(t, nu)) at 50 digits over nu in [3, 10^4] and |t| <= 40: information for DESIGN.md
    section 27, not a gate (the header pins Hill's form itself)."""
    import mpmath as mp
    mp.mp.dps = 50
    worst = (0.0, None)
    for nu in (3, 5, 10, 30, 100, 1000, 10000):
        for t in (0.1, 0.5, 1, 2, 3, 5, 8, 12, 20, 40):
            x = mp.mpf(nu) / (nu + mp.mpf(t) ** 2)
            upper = mp.betainc(mp.mpf(nu) / 2, mp.mpf(1) / 2, 0, x, regularized=True) / 2       # pt(t, nu, lower = FALSE)
            exact = -mp.sqrt(2) * mp.erfinv(2 * upper - 1)
            got = mp.mpf(float(rr.hill_np(np.float64(t), float(nu))))
            dev = float(abs(got - exact) / max(1, abs(exact)))
            if dev > worst[0]:
                worst = (dev, (nu, t))
    print(f"[measure] Hill against the exact z: worst {worst[0]:.3g} relative to max(1, |z|) at (nu, t) = {worst[1]}")
    assert worst[0] < 0.05
