"""plaid.test over several devices: what can be checked without a GPU -- the C ABI declaration, the R shim and wrapper
(R is not installed: statically and with a C compiler against stand-in R headers), and the argument checks that run
before any device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_ARGS, R_ARGS = 15, 12   # plaidhip_plaid_test_multi (include/plaidhip.h), R_plaidhip_plaid_test_multi (.Call routine)


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _args(text, opener):
    """the argument list (top-level commas split) of the first `opener(` ... `)` in text"""
    i = text.index(opener + "(") + len(opener) + 1
    depth, k, cur, out, quote = 1, i, "", [], None
    while True:
        ch = text[k]
        k += 1
        if quote:
            quote = None if ch == quote else quote
        elif ch in "\"'":
            quote = ch
        elif ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                break
        elif ch == "," and depth == 1:
            out.append(cur.strip())
            cur = ""
            continue
        cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _plaid_test_body():
    rsrc = _read("r-pkg", "R", "plaid-hip.R")
    i = rsrc.index("plaid.test <- function(")
    return rsrc[i:rsrc.index("\n}\n", i)]


def test_header_and_signatures_declare_the_entry():
    from plaid_amd import _lib
    header = _read("include", "plaidhip.h")
    assert "int plaidhip_plaid_test_multi(" in header
    assert len(_args(header, "int plaidhip_plaid_test_multi")) == C_ARGS
    assert len(_lib.SIGNATURES["plaidhip_plaid_test_multi"]) == C_ARGS
    assert "plaidhip_debug_plaid_test_sharded_on_one_device" not in header   # a test hook, not API


def test_shim_defines_registers_and_calls_the_entry():
    csrc = _read("r-pkg", "src", "plaidhip_R.c")
    routine = "R_plaidhip_plaid_test_multi"
    params = _args(csrc, "SEXP " + routine)
    assert len(params) == R_ARGS and all(p.startswith("SEXP ") for p in params)
    m = re.search(r'\{"' + routine + r'",\s*\(DL_FUNC\)&' + routine + r",\s*(\d+)\}", csrc)
    assert m and int(m.group(1)) == R_ARGS, "registration"
    body = csrc[csrc.index("SEXP " + routine + "("):]
    body = body[:body.index("\n}\n")]
    assert len(_args(body, "= plaidhip_plaid_test_multi")) == C_ARGS, "the shim passes what the header declares"
    call = [a for a in _args(_plaid_test_body()[_plaid_test_body().index(f'.Call("{routine}"'):], ".Call")
            if not a.startswith("PACKAGE")]
    assert len(call) - 1 == R_ARGS, "the .Call passes what the routine takes"


def test_r_shim_still_compiles():
    out = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                          "-I" + os.path.join(ROOT, "tests", "r_api_stub"), "-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "r-pkg", "src", "plaidhip_R.c")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_r_wrapper_shards_only_with_several_devices():
    """plaid.test(X, y, G, NULL) with options(plaidhip.devices = c(0, 1)) reaches the multi entry, dense X and
    dgCMatrix alike; one device keeps the two single-device routines"""
    body = _plaid_test_body()
    i = body.index('.Call("R_plaidhip_plaid_test_multi"')
    head, branch = body[:i].rsplit("if (length(dev) > 1L", 1)          # the multi route is that branch, nothing else
    assert "else" not in branch and ".Call(" not in branch and "sparse" not in branch, branch
    assert "dev <- .devices()" in head
    tail = body[i:]
    assert '.Call("R_plaidhip_plaid_test_csc", X@p, X@i' in tail and '.Call("R_plaidhip_plaid_test", X,' in tail
    # the dgCMatrix preparation block stays the first test of the class (tests/test_sparse_inputs_host.py)
    k = body.index('inherits(X, "CsparseMatrix")')
    assert body[:k].rstrip().endswith("sparse <-") and k < i


def _small():
    from plaid_amd import synth
    import scipy.sparse as sp
    Gp, Gi = synth.geneset_csc(200, 7, kmin=3, kmax=30)
    X = synth.dense_columns(200, 0, 6)
    Xs = sp.csc_matrix(np.where(X > 9.0, X, 0.0))
    return X, Xs, Gp, Gi


@pytest.mark.parametrize("sparse", [False, True])
def test_bad_arguments_are_refused_before_any_device(sparse):
    """the single-device entries' checks and messages; they fail the same way on a machine without a GPU"""
    import plaid_amd
    X, Xs, Gp, Gi = _small()
    Xin = Xs if sparse else X
    y = np.array([0, 1, 1, 0, 1, 0])
    with pytest.raises(plaid_amd.PlaidHipError, match="elements of y must be 0 or 1"):
        plaid_amd.plaid_test_multi(Xin, np.array([0, 1, 2, 0, 1, 0]), Gp, Gi, devices=2)
    for tests in (0, 8, 15):
        with pytest.raises(plaid_amd.PlaidHipError, match="tests is a bit mask"):
            plaid_amd.plaid_test_multi(Xin, y, Gp, Gi, tests=tests, devices=2)
    with pytest.raises(plaid_amd.PlaidHipError, match="Invalid method"):
        plaid_amd.plaid_test_multi(Xin, y, Gp, Gi, metap_method=2, devices=2)
    with pytest.raises(plaid_amd.PlaidHipError, match="twice"):
        plaid_amd.plaid_test_multi(Xin, y, Gp, Gi, devices=[0, 1, 0])
    with pytest.raises(ValueError):
        plaid_amd.plaid_test_multi(Xin, y[:5], Gp, Gi)
    with pytest.raises(ValueError):
        plaid_amd.plaid_test_multi(Xin, y, Gp, Gi, gsetX=np.zeros((3, 6)))
