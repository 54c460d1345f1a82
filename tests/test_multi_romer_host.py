"""plaid.romer's entries as the header, _lib.SIGNATURES, the R shim, the R wrapper and the Python package declare them,
without a GPU (in the style of tests/test_multi_roast_host.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import roast_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_ARGS = 11   # R_plaidhip_romer (.Call routine)

ENTRIES = {   # the entry -> its C arguments
    "plaidhip_romer": 21, "plaidhip_romer_multi": 22, "plaidhip_dev_romer_keys": 13, "plaidhip_dev_romer_sides": 15,
    "plaidhip_romer_shrink": 7, "plaidhip_romer_finish": 8,
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def _args(text, head):
    """the comma-separated arguments of the first `head(` ... `)` in text"""
    at = text.index(head + "(") + len(head) + 1
    depth, out, cur = 1, [], ""
    while depth:
        ch = text[at]
        at += 1
        if ch in "([":
            depth += 1
        elif ch in ")]":
            depth -= 1
            if depth == 0:
                break
        if ch == "," and depth == 1:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    out.append(cur.strip())
    return [a for a in out if a]


def test_header_and_signatures_declare_the_entries():
    from plaid_amd import _lib
    header = _read("include", "plaidhip.h")
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        assert f"int {name}(" in header
        assert len(_args(header, f"int {name}")) == nargs, name
        assert len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name)
    assert "plaidhip_debug_romer_sharded_on_one_device" not in header            # a test hook, not API
    assert hasattr(lib, "plaidhip_debug_romer_sharded_on_one_device")
    words = header[header.index("plaid.romer(X, design, G, contrasts)"):header.index("int plaidhip_romer(")]
    for word in ("AS RECALLED", "COMPETITIVE", "propTrueNull", "tmixture.vector", "[0.01, 16] / s0^2", "beta'^2 + RSS",
                 "x = t + 0.0", "max(|x|, 1)", "2 (U + 1) - 2 rank_a", "floor(m / 2) + 1", "(b + 1) / (nrot + 1)",
                 "Benjamini-Hochberg", "-Inf < finite < +Inf", "PLAIDHIP_ROAST_MEAN50_MAX", "PLAIDHIP_ROAST_Z_BYTES",
                 "array.weights", "block / correlation", "dgCMatrix", 'na = "fit"', "trend", "robust",
                 "PLAIDHIP_ROMER_MAX_GENES 131072"):
        assert word in words, word
    # the roast block keeps its words and now points here
    roast = header[header.index("plaid.roast(X, design, G, contrasts)"):header.index("int plaidhip_roast(")]
    assert "romer is plaid.romer, below" in roast and "a stated deviation" in roast


def test_shim_defines_registers_and_calls_the_entries():
    csrc = _read("r-pkg", "src", "plaidhip_R.c")
    routine = "R_plaidhip_romer"
    params = _args(csrc, "SEXP " + routine)
    assert len(params) == R_ARGS and all(p.startswith("SEXP ") for p in params)
    m = re.search(r'\{"' + routine + r'",\s*\(DL_FUNC\)&' + routine + r",\s*(\d+)\}", csrc)
    assert m and int(m.group(1)) == R_ARGS, "registration"
    body = csrc[csrc.index("SEXP " + routine + "("):]
    body = body[:body.index("\n}\n")]
    assert len(_args(body, "rc = plaidhip_romer_multi")) == ENTRIES["plaidhip_romer_multi"]
    assert len(_args(body, "rc = plaidhip_romer")) == ENTRIES["plaidhip_romer"]
    rsrc = _read("r-pkg", "R", "plaid-hip.R")
    call = [a for a in _args(rsrc[rsrc.index(f'.Call("{routine}"'):], ".Call") if not a.startswith("PACKAGE")]
    assert len(call) - 1 == R_ARGS, "the .Call passes what the routine takes"
    assert rsrc.count(f'.Call("{routine}"') == 1
    namespace = _read("r-pkg", "NAMESPACE")
    for fn in ("plaid.romer", "plaid.romer.contrasts"):
        assert re.search(r"\b" + re.escape(fn) + r"\b", namespace), fn
        assert f"\n{fn} <- function(" in rsrc, fn
        sig = rsrc[rsrc.index(f"\n{fn} <- function("):]
        sig = sig[:sig.index("{")]
        for word in ('set.statistic = "mean"', "nrot = 9999", "seed = 1", "shrink.resid = TRUE", "rotations = NULL",
                     "minSize = 1", "maxSize = NULL", 'sort.by = "none"'):
            assert word in sig, (fn, word)
    # the R side's option list is the library's, in the library's order
    from plaid_amd import engine
    listed = re.search(r"\.romer_statistics <- c\(([^)]*)\)", rsrc).group(1)
    assert [w.strip().strip('"') for w in listed.split(",")] == sorted(engine.ROMER_STATISTIC, key=engine.ROMER_STATISTIC.get)


def test_r_shim_still_compiles():
    out = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                          "-I" + os.path.join(ROOT, "tests", "r_api_stub"), "-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "r-pkg", "src", "plaidhip_R.c")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_the_constants_agree():
    from plaid_amd import engine
    header = _read("include", "plaidhip.h")
    assert f"#define PLAIDHIP_ROMER_MAX_GENES {engine.ROMER_MAX_GENES}" in header
    assert 2 * engine.ROMER_MAX_GENES < 2 ** 19                        # 2 rank has 19 bits to select on
    romer_h = _read("plaid_amd", "csrc", "romer.h")
    assert "members <= 1024 ? 0 : members <= 16384" in romer_h and engine.ROAST_MEAN50_MAX == 16384
    assert engine.ROAST_MEAN50_MAX * 4 <= 64 * 1024                    # a wave's 2 rank of the largest set in LDS
    kern = _read("plaid_amd", "csrc", "kernels_romer.hip")
    assert "for (int bit = 18; bit >= 0; --bit)" in kern


def test_python_exports():
    import plaid_amd
    for name in ("plaid_romer", "plaid_romer_contrasts", "romer_multi"):
        assert name in plaid_amd.__all__ and callable(getattr(plaid_amd, name))
    assert callable(plaid_amd.Context.romer)
    from plaid_amd import engine
    assert engine.ROMER_COLUMNS == ("NGenes", "Up", "Down", "Mixed", "FDR.Up", "FDR.Down", "FDR.Mixed")


def test_the_device_list_is_checked_before_anything_else():
    import plaid_amd
    from plaid_amd import engine
    rng = np.random.default_rng(1)
    X = rng.normal(size=(8, 10))
    D = rr.make_design(10, 2, rng)
    with pytest.raises(plaid_amd.PlaidHipError, match="twice"):
        engine.romer_multi(X, D, [0, 2], [0, 1], devices=[0, 1, 0])
    with pytest.raises(plaid_amd.PlaidHipError, match="ndev"):
        engine.romer_multi(X, D, [0, 2], [0, 1], devices=[])
    with pytest.raises(ValueError):
        engine.romer_multi(X, D, [0, 2], [0, 1], devices=None)
