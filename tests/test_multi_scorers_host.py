"""replaid.ucell / aucell / scse / gsva over several devices: what can be checked without a GPU -- the C ABI declarations,
the R shim and wrappers (R is not installed: statically and with a C compiler against stand-in R headers), and the
argument checks that run before any device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("ucell", "aucell", "scse", "gsva")
# arguments of plaidhip_<method>_multi (include/plaidhip.h) and of the R_plaidhip_<method>_multi .Call routine
C_ARGS = {"ucell": 13, "aucell": 12, "scse": 14, "gsva": 13}
R_ARGS = {"ucell": 10, "aucell": 9, "scse": 10, "gsva": 10}


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


def _r_function(rsrc, name):
    """the body of `name <- function(...) {...}` in the R source"""
    i = rsrc.index(name + " <- function(")
    j = rsrc.index("\n}\n", i)
    return rsrc[i:j]


@pytest.mark.parametrize("method", METHODS)
def test_header_declares_the_multi_entry(method):
    header = _read("include", "plaidhip.h")
    assert f"int plaidhip_{method}_multi(" in header
    assert len(_args(header, f"int plaidhip_{method}_multi")) == C_ARGS[method]


@pytest.mark.parametrize("method", METHODS)
def test_shim_defines_registers_and_calls_the_multi_entry(method):
    csrc = _read("r-pkg", "src", "plaidhip_R.c")
    routine = f"R_plaidhip_{method}_multi"
    params = _args(csrc, "SEXP " + routine)
    assert len(params) == R_ARGS[method] and all(p.startswith("SEXP ") for p in params)
    m = re.search(r'\{"' + routine + r'",\s*\(DL_FUNC\)&' + routine + r",\s*(\d+)\}", csrc)
    assert m and int(m.group(1)) == R_ARGS[method], "registration"
    body = csrc[csrc.index("SEXP " + routine + "("):]
    body = body[:body.index("\n}\n")]
    assert len(_args(body, f"check(plaidhip_{method}_multi")) == C_ARGS[method], "the shim passes what the header declares"
    rsrc = _read("r-pkg", "R", "plaid-hip.R")
    call = [a for a in _args(rsrc[rsrc.index(f'.Call("{routine}"'):], ".Call") if not a.startswith("PACKAGE")]
    assert len(call) - 1 == R_ARGS[method], "the .Call passes what the routine takes"


@pytest.mark.parametrize("method", METHODS)
def test_r_wrapper_shards_only_with_several_devices(method):
    rsrc = _read("r-pkg", "R", "plaid-hip.R")
    body = _r_function(rsrc, f"replaid.{method}")
    i = body.index(f'.Call("R_plaidhip_{method}_multi"')
    head, branch = body[:i].rsplit("if (length(dev) > 1L", 1)          # the multi route is that branch, nothing else
    assert "else" not in branch and ".Call(" not in branch, branch
    assert "dev <- .devices()" in head
    if method == "gsva":
        assert '"ecdf"' in branch.split("{")[0], "gsva's multi route must exclude rowtf = ecdf"
        assert '.Call("R_plaidhip_gsva",' in body and '.Call("R_plaidhip_gsva_csc",' in body
    else:
        assert f'.Call("R_plaidhip_{method}",' in body, "the single-device route stays"


def test_r_shim_still_compiles():
    out = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                          "-I" + os.path.join(ROOT, "tests", "r_api_stub"), "-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "r-pkg", "src", "plaidhip_R.c")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def _small():
    from plaid_amd import synth
    Gp, Gi = synth.geneset_csc(200, 7, kmin=3, kmax=30)
    X = synth.dense_columns(200, 0, 5)
    return X, Gp, Gi


def test_bad_arguments_are_refused_before_any_device():
    """argument checks run before a context is created: they fail the same way on a machine without a GPU"""
    import plaid_amd
    X, Gp, Gi = _small()
    with pytest.raises(plaid_amd.PlaidHipError, match="rmax must be positive"):
        plaid_amd.ucell_multi(X, Gp, Gi, np.diff(Gp), rmax=0)
    with pytest.raises(plaid_amd.PlaidHipError, match="aucMaxRank must be positive"):
        plaid_amd.aucell_multi(X, Gp, Gi, 0)
    with pytest.raises(plaid_amd.PlaidHipError, match="ecdf"):
        plaid_amd.gsva_multi(X, Gp, Gi, rowtf="ecdf", devices=2)
    with pytest.raises(ValueError):
        plaid_amd.gsva_multi(X, Gp, Gi, rowtf="rank")
