"""plaid.camera over several devices: what can be checked without a GPU -- the C ABI declarations, the R shim and wrappers
(R is not installed: statically and with a C compiler against stand-in R headers), the device list's own checks, and that
the numpy restatement's deviation from the 50-digit form is what the GPU test's allowance was taken from.  (The engine's
worker threads, its rendezvous and the chained sums need a device: tests/test_gpu_camera.py runs them on the hook.)"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import camera_ref as cr
from tests.test_multi_plaid_test_host import ROOT, _args, _read

ENTRIES = {   # the entry -> its C arguments
    "plaidhip_camera": 17, "plaidhip_camera_multi": 18, "plaidhip_dev_camera_residuals": 15, "plaidhip_dev_camera_sumsq": 7,
    "plaidhip_camera_residual_row": 9, "plaidhip_camera_finish": 15,
}
R_ARGS = 10   # R_plaidhip_camera (.Call routine)


def test_header_and_signatures_declare_the_entries():
    from plaid_amd import _lib
    header = _read("include", "plaidhip.h")
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        assert f"int {name}(" in header
        assert len(_args(header, f"int {name}")) == nargs, name
        assert len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name)
    assert "plaidhip_debug_camera_sharded_on_one_device" not in header   # a test hook, not API
    assert hasattr(lib, "plaidhip_debug_camera_sharded_on_one_device")
    for word in ("use.ranks", "trend.var", "weights", "dgCMatrix", 'na = "fit"', "fry / roast"):
        assert word in header[header.index("plaid.camera(X, design, G, contrasts)"):header.index("int plaidhip_camera(")], word


def test_shim_defines_registers_and_calls_the_entries():
    csrc = _read("r-pkg", "src", "plaidhip_R.c")
    routine = "R_plaidhip_camera"
    params = _args(csrc, "SEXP " + routine)
    assert len(params) == R_ARGS and all(p.startswith("SEXP ") for p in params)
    m = re.search(r'\{"' + routine + r'",\s*\(DL_FUNC\)&' + routine + r",\s*(\d+)\}", csrc)
    assert m and int(m.group(1)) == R_ARGS, "registration"
    body = csrc[csrc.index("SEXP " + routine + "("):]
    body = body[:body.index("\n}\n")]
    assert len(_args(body, "rc = plaidhip_camera_multi")) == ENTRIES["plaidhip_camera_multi"]
    assert len(_args(body, "rc = plaidhip_camera")) == ENTRIES["plaidhip_camera"]
    rsrc = _read("r-pkg", "R", "plaid-hip.R")
    call = [a for a in _args(rsrc[rsrc.index(f'.Call("{routine}"'):], ".Call") if not a.startswith("PACKAGE")]
    assert len(call) - 1 == R_ARGS, "the .Call passes what the routine takes"
    assert rsrc.count(f'.Call("{routine}"') == 1                      # one way in for the three R functions
    namespace = _read("r-pkg", "NAMESPACE")
    for fn in ("plaid.camera", "plaid.camera.contrasts", "plaid.intergenecor"):
        assert re.search(r"\b" + re.escape(fn) + r"\b", namespace), fn
        assert f"\n{fn} <- function(" in rsrc, fn


def test_r_shim_still_compiles():
    out = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                          "-I" + os.path.join(ROOT, "tests", "r_api_stub"), "-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "r-pkg", "src", "plaidhip_R.c")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_python_exports():
    import plaid_amd
    for name in ("plaid_camera", "plaid_camera_contrasts", "plaid_intergenecor", "camera_multi"):
        assert name in plaid_amd.__all__ and callable(getattr(plaid_amd, name))
    assert callable(plaid_amd.Context.camera)


def test_the_device_list_is_checked_before_anything_else():
    import plaid_amd
    from plaid_amd import engine
    rng = np.random.default_rng(1)
    X = cr.int_matrix(8, 10, rng)
    D = cr.make_design(10, 2, rng)
    with pytest.raises(plaid_amd.PlaidHipError, match="twice"):
        engine.camera_multi(X, D, [0, 2], [0, 1], devices=[0, 1, 0])
    with pytest.raises(plaid_amd.PlaidHipError, match="ndev"):
        engine.camera_multi(X, D, [0, 2], [0, 1], devices=[])
    with pytest.raises(ValueError):
        engine.camera_multi(X, D, [0, 2], [0, 1], devices=None)


def test_the_numpy_restatement_deviates_by_what_the_gpu_test_allows_eight_times():
    """camera_np (the pinned order in plain fp64) against camera_mp (limma's literal form at 50 digits) over the end-to-end
    cases: the figures tests/test_gpu_camera.py records as MEASURED, re-measured here.  Rounding in a fixed order is all that
    separates the two, so the figures are stable to the libm and BLAS at hand within a small factor: 2 is asserted."""
    from tests.test_gpu_camera import MEASURED
    worst = {k: 0.0 for k in MEASURED}
    for name in cr.E2E_CASES:
        for mode in cr.E2E_MODES:
            ref, got = cr.e2e_reference(name, mode, "mp"), cr.e2e_reference(name, mode, "np")
            for f in range(len(ref)):
                for j in range(len(ref[f])):
                    dev = cr.deviation(got[f][j], ref[f][j])
                    for k in worst:
                        worst[k] = max(worst[k], dev[k])
    print("[measure] camera_np against camera_mp: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 2 * MEASURED[k], (k, v)
        assert v > 0
