"""replaid.gsva (rowtf "z" and "ecdf"; dense and dgCMatrix X; one shard or several) against the exact reference of
tests/helpers/gsva_ref.py, at its derived fp64 bound -- `pytest -m gpu`.

A gsva score is a mean of signed ranks over max|rank|: one member whose rank is off by 1/2, or whose sign is -1 where
it is 0, moves a score by ~1 / (2 k g), far below any relative tolerance but >= 4 x the bound here
(tests/test_gsva_rank_ref.py shows both, on the host).  The ranks follow a real-valued row transform, so the comparison
needs the inputs' |z| to be separated by more than the transform's own error: gsva_ref.separated(), asserted for every
input below (and, with its margins, in the host file).  The ties that remain are declared: two bit-identical genes, a
constant gene (value 1.25, a member of set 0 and of a singleton set: its z, sign and weight are exactly 0) and an
all-zero dgCMatrix row.

The constant gene is what the dense route used to miss: it formed the row mean as sum * fl(1 / n), which is not 1.25
for n = 105, 117, 123, ... -- z = -2e-8, signed rank -1.  On the parent of this file's commit the dense n = 105 cases
(and the dense entry of the n = 117 dgCMatrix case) fail here; the mean is now a true division, as in the dgCMatrix
branch and in R's rowMeans.

Every test prints the largest |error| / bound it met (`pytest -s`)."""
import functools

import numpy as np
import pytest

from tests.helpers import exact_ref as er
from tests.helpers import gsva_cases as gc
from tests.helpers import gsva_ref as gr
from tests.helpers import sharded_hooks

pytestmark = pytest.mark.gpu
GSVA = sharded_hooks.GSVA


@functools.lru_cache(maxsize=None)
def _ambiguous(kind, name):
    X, ties = gc.z_input(kind, name)
    return gr.separated(gr.z_exact(X), gr.z_delta(X), ties)[0]


def _within(got, kind, name, tau, rowtf, what):
    N, B, _, _, _ = gc.gsva_reference(kind, name, tau, rowtf)
    print(f"RATIO gsva {what} {name} tau={tau}: {gr.ratio(got, N, B):.3g}")
    er.assert_within(got, N, B, f"gsva {what} {name} tau={tau}")


def _declared_rows(got, Gp, ties):
    """the singleton sets of the declared genes are the last rows, in gene order: bit-identical genes score alike"""
    force = sorted(r for grp in ties for r in grp)
    first = len(Gp) - 1 - len(force)
    for grp in ties:
        rows = [first + force.index(r) for r in grp]
        for r in rows[1:]:
            er.assert_same_bits(got[r], got[rows[0]], f"identical genes {grp}")


@pytest.mark.parametrize("tau", gc.TAUS)
@pytest.mark.parametrize("name", list(gc.DENSE))
def test_gsva_dense_z_within_the_bound(hip_ctx, name, tau):
    """the rank kernel's size classes (g = 257 ... 20449, n = 5 ... 9) and the column-block seams of the row moments
    (n = 105 ... 300 at g = 600), exponents 1, 1.5 and 1.3"""
    assert _ambiguous("dense", name) == 0
    X, Gp, Gi, ties = gc.dense_case(name)
    S = hip_ctx.gsva(X, Gp, Gi, tau, "z")
    _within(S, "dense", name, tau, "z", "dense z")
    _declared_rows(S, Gp, ties)


def test_gsva_dense_z_tau_075_within_the_bound_of_its_larger_allowance(hip_ctx):
    """tau = 0.75: the exponent 1.75 is pow_quarters' q = 7, whose weights exceed 3 u by IEEE operations alone (3.90 u over
    every rank, tests/test_pow_ref.py): held at the c = 5 + 2 * 4.5 that pow_ref.pow_allowance_u(1.75) gives, at the
    12,289-row size class"""
    from tests.helpers.pow_ref import pow_allowance_u
    assert pow_allowance_u(1.75) == 4.5
    name, tau = "g12289", 0.75
    assert _ambiguous("dense", name) == 0
    X, Gp, Gi, ties = gc.dense_case(name)
    S = hip_ctx.gsva(X, Gp, Gi, tau, "z")
    _within(S, "dense", name, tau, "z", "dense z")
    _declared_rows(S, Gp, ties)


@pytest.mark.parametrize("tau", gc.TAUS)
@pytest.mark.parametrize("name", list(gc.CSC))
def test_gsva_csc_z_within_the_bound_and_so_is_the_dense_entry(hip_ctx, name, tau):
    """the row view of a dgCMatrix (transpose, row moments on either side of a wavefront's 64 entries and of kLongRow =
    4096, the implicit zeros' default z, the expansion): stored zeros, negative values, an all-zero gene, a gene stored
    in every cell, a constant stored gene, an empty cell.  The dense entry on toarray() is held to the SAME reference:
    the two routes agree within twice the bound, and on every rank"""
    assert _ambiguous("csc", name) == 0
    Xs, Gp, Gi, ties = gc.csc_case(name)
    g = Xs.shape[0]
    S = hip_ctx.gsva_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, tau, "z")
    _within(S, "csc", name, tau, "z", "csc z")
    _declared_rows(S, Gp, ties)
    D = hip_ctx.gsva(Xs.toarray(), Gp, Gi, tau, "z")
    _within(D, "csc", name, tau, "z", "dense entry of csc z")


@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("name", list(gc.CSC))
def test_gsva_csc_ecdf_within_the_bound_and_bitwise_the_dense_entry(hip_ctx, name, tau):
    """rowtf = "ecdf" ranks the integer counts #{x <= x_i} of a gene's row (values rounded to one decimal: ties inside
    the rows): exact on every route, so the dgCMatrix entry has the dense entry's bits, and both are within the bound"""
    Xs, Gp, Gi, ties = gc.csc_case(name, rounded=True)
    g = Xs.shape[0]
    S = hip_ctx.gsva_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, tau, "ecdf")
    D = hip_ctx.gsva(Xs.toarray(), Gp, Gi, tau, "ecdf")
    er.assert_same_bits(S, D, "ecdf: the dgCMatrix entry against the dense entry")
    _within(S, "csc", name, tau, "ecdf", "csc ecdf")
    _declared_rows(S, Gp, ties)


@pytest.mark.parametrize("nshards", [2, 3])
def test_gsva_sharded_within_the_same_bound(hip_ctx, nshards):
    """2 and 3 shards on one device (the engine's test hook): every sharding within the bound of the one reference.
    Dense X chains its row moments in the one-device order: the one-device bits, as promised.  A dgCMatrix adds the
    shards' row sums on the host, in another order than one device does: the bound, not the bits"""
    for name in gc.SHARDED_DENSE:
        assert _ambiguous("dense", name) == 0
        X, Gp, Gi, _ = gc.dense_case(name)
        for tau in gc.TAUS:
            rc, S, _ = sharded_hooks.scorer(nshards, GSVA, X, Gp, Gi, tau=tau)
            assert rc == 0
            _within(S, "dense", name, tau, "z", f"dense z {nshards} shards")
            er.assert_same_bits(S, hip_ctx.gsva(X, Gp, Gi, tau, "z"), f"{name}: {nshards} shards against one device")
    for name in gc.SHARDED_CSC:
        assert _ambiguous("csc", name) == 0
        Xs, Gp, Gi, ties = gc.csc_case(name)
        for tau in gc.TAUS:
            rc, S, _ = sharded_hooks.scorer(nshards, GSVA, Xs, Gp, Gi, tau=tau)
            assert rc == 0
            _within(S, "csc", name, tau, "z", f"csc z {nshards} shards")
            _declared_rows(S, Gp, ties)
