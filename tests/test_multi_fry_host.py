"""plaid.fry over several devices: what can be checked without a GPU -- the C ABI declarations, the R shim and wrappers (R is
not installed: statically and with a C compiler against stand-in R headers), the device list's own checks, and that the
numpy restatement's deviation from the 50-digit form is what the GPU test's allowance was taken from."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import camera_ref as cr
from tests.helpers import fry_ref as fr
from tests.test_multi_plaid_test_host import ROOT, _args, _read

ENTRIES = {   # the entry -> its C arguments
    "plaidhip_fry": 16, "plaidhip_fry_multi": 17, "plaidhip_dev_fry_residuals": 14, "plaidhip_dev_fry_residual_effects": 10,
    "plaidhip_dev_fry_gram": 14, "plaidhip_dev_fry_eigen": 9, "plaidhip_fry_q2": 7, "plaidhip_fry_divisors": 7,
    "plaidhip_fry_residual_row": 8, "plaidhip_fry_finish": 14,
}
R_ARGS = 9   # R_plaidhip_fry (.Call routine)


def test_header_and_signatures_declare_the_entries():
    from plaid_amd import _lib
    header = _read("include", "plaidhip.h")
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        assert f"int {name}(" in header
        assert len(_args(header, f"int {name}")) == nargs, name
        assert len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name)
    for hookname in ("plaidhip_debug_fry_sharded_on_one_device", "plaidhip_debug_beta_upper"):
        assert hookname not in header and hasattr(lib, hookname)       # test hooks, not API
    words = header[header.index("plaid.fry(X, design, G, contrasts)"):header.index("int plaidhip_fry(")]
    for word in ("AS RECALLED", "posterior.sd", "roast and mroast", "weights", "trend.var", "dgCMatrix", 'na = "fit"', '"p2"',
                 "PLAIDHIP_FRY_MIXED_MAX 128", "2 pt(-|t|, d)", "BY INDEX"):
        assert word in words, word
    camera = header[header.index("plaid.camera(X, design, G, contrasts)"):header.index("int plaidhip_camera(")]
    assert "fry / roast" in camera                                      # plaid.camera itself still does not offer it


def test_shim_defines_registers_and_calls_the_entries():
    csrc = _read("r-pkg", "src", "plaidhip_R.c")
    routine = "R_plaidhip_fry"
    params = _args(csrc, "SEXP " + routine)
    assert len(params) == R_ARGS and all(p.startswith("SEXP ") for p in params)
    m = re.search(r'\{"' + routine + r'",\s*\(DL_FUNC\)&' + routine + r",\s*(\d+)\}", csrc)
    assert m and int(m.group(1)) == R_ARGS, "registration"
    body = csrc[csrc.index("SEXP " + routine + "("):]
    body = body[:body.index("\n}\n")]
    assert len(_args(body, "rc = plaidhip_fry_multi")) == ENTRIES["plaidhip_fry_multi"]
    assert len(_args(body, "rc = plaidhip_fry")) == ENTRIES["plaidhip_fry"]
    rsrc = _read("r-pkg", "R", "plaid-hip.R")
    call = [a for a in _args(rsrc[rsrc.index(f'.Call("{routine}"'):], ".Call") if not a.startswith("PACKAGE")]
    assert len(call) - 1 == R_ARGS, "the .Call passes what the routine takes"
    assert rsrc.count(f'.Call("{routine}"') == 1
    namespace = _read("r-pkg", "NAMESPACE")
    for fn in ("plaid.fry", "plaid.fry.contrasts"):
        assert re.search(r"\b" + re.escape(fn) + r"\b", namespace), fn
        assert f"\n{fn} <- function(" in rsrc, fn


def test_r_shim_still_compiles():
    out = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                          "-I" + os.path.join(ROOT, "tests", "r_api_stub"), "-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "r-pkg", "src", "plaidhip_R.c")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_python_exports():
    import plaid_amd
    for name in ("plaid_fry", "plaid_fry_contrasts", "fry_multi"):
        assert name in plaid_amd.__all__ and callable(getattr(plaid_amd, name))
    assert callable(plaid_amd.Context.fry)


def test_the_device_list_is_checked_before_anything_else():
    import plaid_amd
    from plaid_amd import engine
    rng = np.random.default_rng(1)
    X = cr.int_matrix(8, 10, rng)
    D = cr.make_design(10, 2, rng)
    with pytest.raises(plaid_amd.PlaidHipError, match="twice"):
        engine.fry_multi(X, D, [0, 2], [0, 1], devices=[0, 1, 0])
    with pytest.raises(plaid_amd.PlaidHipError, match="ndev"):
        engine.fry_multi(X, D, [0, 2], [0, 1], devices=[])
    with pytest.raises(ValueError):
        engine.fry_multi(X, D, [0, 2], [0, 1], devices=None)


def test_the_numpy_restatement_deviates_by_what_the_gpu_test_allows_four_times():
    """fry_np (lstsq, numpy's complete QR, eigvalsh, scipy's tails) against fry_mp over the end-to-end cases and the three
    `standardize` values: the figures fry_ref.MEASURED records, re-measured here.  Rounding is all that separates the two,
    so the figures are stable to the libm and LAPACK at hand within a small factor: 2 is asserted."""
    worst, kept, total = fr.measure_np()
    print("[measure] fry_np against fry_mp: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"; {kept} of {total} conditioned")
    for k, v in worst.items():
        assert v <= 2 * fr.MEASURED[k], (k, v)
        assert v > 0


def test_eigvalsh_deviates_by_what_the_eigen_certificate_allows_four_times():
    """numpy.linalg.eigvalsh against the 50-digit spectrum over the eigen cases (the D = 128 pair from tests/golden): the
    figure fry_ref.EIG_DEV records"""
    import mpmath as mp
    worst = 0.0
    with mp.workdps(fr.DPS + 20):
        for name, (M, Dn) in fr.eigen_cases().items():
            e1, eD = fr.eigen_exact(name)
            lam = np.sort(np.linalg.eigvalsh(M))[::-1]
            worst = max(worst, float(max(abs(mp.mpf(lam[0]) - e1), abs(mp.mpf(lam[Dn - 1]) - eD)) / e1))
        gold = np.load(os.path.join(ROOT, "tests", "golden", "fry_eig128.npz"))
        assert int(gold["seed"]) == fr.EIG128_SEED
        e1, eD = mp.mpf(str(gold["lam1"][0])), mp.mpf(str(gold["lam128"][0]))
        lam = np.sort(np.linalg.eigvalsh(fr.eig128_matrix()))[::-1]
        worst = max(worst, float(max(abs(mp.mpf(lam[0]) - e1), abs(mp.mpf(lam[127]) - eD)) / e1))
    print(f"[measure] eigvalsh against 50 digits: {worst:.3g}")
    assert 0 < worst <= 2 * fr.EIG_DEV
