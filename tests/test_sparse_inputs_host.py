"""replaid.gsva / plaid.test on a dgCMatrix (plaidhip_gsva_csc / plaidhip_plaid_test_csc): the declarations, the ctypes
table and the R wrappers agree, and the R wrappers send a sparse X as its slots.  No GPU needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_header_and_ctypes_table_declare_the_csc_entries():
    from plaid_amd import _lib
    hdr = _read("include", "plaidhip.h")
    for name, nargs in (("plaidhip_gsva_csc", 12), ("plaidhip_plaid_test_csc", 14)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/plaidhip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs


def _function_body(src, name):
    start = src.index(name + " <- function(")
    nxt = re.search(r"\n[A-Za-z.][A-Za-z0-9._]* <- function\(", src[start + 1:])
    return src[start:start + 1 + nxt.start()] if nxt else src[start:]


def _sparse_branch(body):
    """the lines of the CsparseMatrix branch: from the inherits() test to the matching else"""
    k = body.index('inherits(X, "CsparseMatrix")')
    depth, out = 0, []
    for line in body[k:].splitlines()[1:]:
        depth += line.count("{") - line.count("}")
        if depth < 0 or line.strip().startswith("} else"):
            break
        out.append(line)
    return "\n".join(out)


def test_r_wrappers_send_a_dgcmatrix_as_its_slots():
    src = _read("r-pkg", "R", "plaid-hip.R")
    gsva = _function_body(src, "replaid.gsva")
    branch = _sparse_branch(gsva)
    assert '"R_plaidhip_gsva_csc"' in branch and "X@p" in branch and "X@i" in branch
    assert "as.matrix" not in branch
    pt = _function_body(src, "plaid.test")
    branch = _sparse_branch(pt)
    assert "X[gg, , drop = FALSE]" in branch and "as.matrix" not in branch
    assert '"R_plaidhip_plaid_test_csc", X@p, X@i' in pt
    shim = _read("r-pkg", "src", "plaidhip_R.c")
    for name, nargs in (("R_plaidhip_gsva_csc", 8), ("R_plaidhip_plaid_test_csc", 10)):
        assert re.search(r'\{"' + name + r'", \(DL_FUNC\)&' + name + r", " + str(nargs) + r"\}", shim)
