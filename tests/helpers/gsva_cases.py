"""The inputs of the gsva / aucell / scse bound tests: one table for the host file (tests/test_gsva_rank_ref.py, which
asserts the separation precondition of every z input) and for the GPU files.  Host only; everything is built from a seed
and cached.  A seed is chosen so that tests/helpers/gsva_ref.separated() holds with margin; another seed, not a wider
bound, is the answer where it does not."""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

CONST = 1.25            # the constant gene: its row sum 1.25 n is exact, so is its mean under a true division
TAUS = (0.0, 0.5, 0.3)  # exponents 1 (exact fp32 staging), 1.5 (pow_quarters), 1.3 (pow())


def sets(g, m, seed, kmin=2, kmax=300, force=()):
    """m sets of kmin ... kmax genes (both met), then one singleton per gene of `force`; set 0 also holds `force`"""
    rng = np.random.default_rng(seed)
    kmax = min(kmax, g)
    sizes = rng.integers(kmin, kmax + 1, size=m)
    sizes[0], sizes[-1] = kmax, kmin
    members = [np.sort(rng.choice(g, size=int(s), replace=False)) for s in sizes]
    if len(force):
        members[0] = np.union1d(members[0], np.asarray(force))
    members += [np.array([f]) for f in force]
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in members])]).astype(np.int32)
    Gi = np.concatenate(members).astype(np.int32)
    return Gp, Gi


# ------------------------------------------------------------------ dense X for rowtf = "z"
# (g, n, seed): the rank kernel's size classes at n = 5 ... 9, then the column-block seams of kRowColBlock = 128 (and 300 for
# the shards) at g = 600; n = 105 is where fl(1 / n) * (1.25 n) != 1.25
DENSE = {
    "g257": (257, 5, 1), "g2049": (2049, 6, 2), "g8193": (8193, 7, 3), "g12289": (12289, 8, 4), "g20449": (20449, 9, 5),
    "n105": (600, 105, 6), "n127": (600, 127, 7), "n128": (600, 128, 8), "n129": (600, 129, 9), "n257": (600, 257, 10),
    "n300": (600, 300, 11),
}
DENSE_TIES = ([0, 1], [2])          # genes 0 / 1 bit-identical, gene 2 constant


@functools.lru_cache(maxsize=None)
def dense_case(name):
    """(X, Gp, Gi, tie_groups): gamma(2, 1.5) data with two bit-identical genes (0, 1), the constant gene 2 (1.25, a
    member of set 0 and of a singleton set) and two identical samples (the first and the last)"""
    g, n, seed = DENSE[name]
    rng = np.random.default_rng(seed)
    X = rng.gamma(2.0, 1.5, size=(g, n))
    X[1, :] = X[0, :]
    X[2, :] = CONST
    X[:, n - 1] = X[:, 0]
    Gp, Gi = sets(g, 200 if g > 600 else 60, seed + 100, force=(0, 1, 2))
    X = np.asfortranarray(X)
    X.setflags(write=False)
    return X, Gp, Gi, DENSE_TIES


# ------------------------------------------------------------------ dgCMatrix X
def _with_stored_zeros(X, pairs):
    """CSC of X that also stores the (row, column) pairs where X is zero"""
    Xs = sp.csc_matrix(X)
    r, c = np.asarray(pairs, dtype=np.int64).T
    keep = X[r, c] == 0.0
    coo = Xs.tocoo()
    out = sp.csc_matrix((np.concatenate([coo.data, np.zeros(int(keep.sum()))]),
                         (np.concatenate([coo.row, r[keep]]), np.concatenate([coo.col, c[keep]]))), shape=X.shape)
    out.sort_indices()
    assert out.nnz > Xs.nnz
    return out


def _edge(rounded, seed, g=2000, n=300):
    """~90 % zeros with the edge cases of the row view: genes 0 / 1 identical, gene 2 all zero, gene 3 stored in every
    cell but the empty one, cell 5 empty, explicit stored zeros, negative values in a tenth of the genes"""
    rng = np.random.default_rng(seed)
    X = rng.gamma(2.0, 1.5, size=(g, n))
    if rounded:
        X = np.round(X, 1)
    X[rng.random(X.shape) < 0.9] = 0.0
    neg = rng.random(g) < 0.1
    X[neg, :] *= np.where(rng.random((int(neg.sum()), n)) < 0.5, -1.0, 1.0)
    X[1, :] = X[0, :]
    X[2, :] = 0.0
    X[3, :] = rng.gamma(2.0, 1.5, size=n) + 0.05
    if rounded:
        X[3, :] = np.round(X[3, :], 1)
    X[:, 5] = 0.0
    return _with_stored_zeros(X, [(10, 0), (11, 1), (12, 2), (40, 7), (41, 7), (2, 9)]), ([0, 1], [2])


def _const(rounded, seed, g=300, n=117):
    """a small matrix, ~80 % zeros, with a constant gene STORED in every cell (gene 2; short rows: the wavefront path),
    two identical genes and an all-zero one.  n = 117: fl(1 / n) * (1.25 n) != 1.25 here too"""
    rng = np.random.default_rng(seed)
    X = rng.gamma(2.0, 1.5, size=(g, n))
    if rounded:
        X = np.round(X, 1)
    X[rng.random(X.shape) < 0.8] = 0.0
    X[1, :] = X[0, :]
    X[2, :] = CONST
    X[3, :] = 0.0
    return _with_stored_zeros(X, [(10, 0), (11, 1), (3, 9)]), ([0, 1], [2], [3])


def _long(rounded, seed, g=300, n=4200):
    """rows of 64, 65, 4096 and 4097 stored entries (genes 10 ... 13: either side of a wavefront's width and of
    kLongRow), a constant gene stored in all 4,200 cells (gene 2: the workgroup-per-row path), ~90 % zeros elsewhere"""
    rng = np.random.default_rng(seed)
    X = rng.gamma(2.0, 1.5, size=(g, n)) + 0.05
    if rounded:
        X = np.round(X, 1)
    X[rng.random(X.shape) < 0.9] = 0.0
    for row, cnt in zip((10, 11, 12, 13), (64, 65, 4096, 4097)):
        v = rng.gamma(2.0, 1.5, size=n) + 0.05
        v = np.round(v, 1) if rounded else v
        v[rng.permutation(n)[cnt:]] = 0.0
        X[row, :] = v
    X[1, :] = X[0, :]
    X[2, :] = CONST
    Xs = sp.csc_matrix(X)
    Xs.sort_indices()
    assert [int(c) for c in np.diff(Xs.tocsr().indptr)[10:14]] == [64, 65, 4096, 4097]
    return Xs, ([0, 1], [2])


CSC = {"edge": (_edge, 11), "const": (_const, 12), "long": (_long, 15)}


@functools.lru_cache(maxsize=None)
def csc_case(name, rounded=False):
    """(Xs, Gp, Gi, tie_groups): continuous values for "z", values rounded to one decimal (ties inside a gene's row) for
    "ecdf".  The declared genes are members of set 0 and of singleton sets"""
    make, seed = CSC[name]
    Xs, ties = make(rounded, seed + (50 if rounded else 0))
    g = Xs.shape[0]
    force = tuple(sorted(r for grp in ties for r in grp))
    # (4,200 samples: smaller sets keep the exact sums of the reference quick)
    Gp, Gi = sets(g, 40, seed + 200, kmax=40, force=force) if name == "long" else sets(g, 60, seed + 200, force=force)
    return Xs, Gp, Gi, ties


# every (kind, name) whose z transform the GPU tests run: dense entry, CSC entry, and the sharded runs of both
Z_INPUTS = [("dense", k) for k in DENSE] + [("csc", k) for k in CSC]
SHARDED_DENSE = ("n129", "n300")
SHARDED_CSC = ("edge",)


def z_input(kind, name):
    """(dense X, tie_groups) of one z input"""
    if kind == "dense":
        X, _, _, ties = dense_case(name)
        return X, ties
    Xs, _, _, ties = csc_case(name)
    return Xs.toarray(), ties


@functools.lru_cache(maxsize=None)
def gsva_reference(kind, name, tau, rowtf="z"):
    """(N, B, T, E, wmax) of one input, computed once for every test that needs it: gsva_ref's normalised reference and
    bound, gsva_raw_ref's raw scores, their bound and the largest |weight|.  rowtf "ecdf" takes the rounded CSC matrix"""
    from tests.helpers import gsva_ref as gr
    if kind == "dense":
        X, Gp, Gi, _ = dense_case(name)
    else:
        Xs, Gp, Gi, _ = csc_case(name, rounded=rowtf == "ecdf")
        X = Xs.toarray()
    T, E, wmax = gr.gsva_raw_ref(X, Gp, Gi, tau, rowtf)
    N, B = gr.gsva_ref(X, Gp, Gi, tau, rowtf, raw=(T, E))
    for a in (N, B, T, E):
        a.setflags(write=False)
    return N, B, T, E, wmax


# ------------------------------------------------------------------ replaid.aucell
AUCELL_G = (257, 20449)


def aucell_ks(g):
    """K = 1, the default ceil(0.05 g), g, and g + 7 (more than there are genes)"""
    return (1.0, float(np.ceil(0.05 * g)), float(g), float(g + 7))


@functools.lru_cache(maxsize=None)
def aucell_case(g, sparse):
    """(X, Gp, Gi): n = 6 columns of values rounded to one decimal (ties everywhere), and tie groups placed astride the
    thresholds max - K: column 0 ties the six values around position g - ceil(0.05 g) of its order, column 1 ties its two
    largest values (K = 1: the top rank becomes g - 1/2), column 2 has a unique maximum (max(r) = g).  sparse: ~85 %
    zeros that tie at the bottom, as a scipy CSC matrix"""
    rng = np.random.default_rng(g + int(sparse))
    n = 6
    X = np.round(rng.gamma(2.0, 1.5, size=(g, n)), 1) + 0.1
    if sparse:
        X[rng.random(X.shape) < 0.85] = 0.0
    K = int(np.ceil(0.05 * g))
    o = np.argsort(X[:, 0], kind="stable")
    X[o[g - K - 3:g - K + 3], 0] = X[o[g - K], 0]
    o = np.argsort(X[:, 1], kind="stable")
    X[o[-2:], 1] = X[o[-1], 1] + 1.0
    o = np.argsort(X[:, 2], kind="stable")
    X[o[-1], 2] += 1.0
    Gp, Gi = sets(g, 120, g + 7, kmin=1, kmax=min(g, 300), force=(int(o[-1]),))
    return (sp.csc_matrix(X) if sparse else np.asfortranarray(X)), Gp, Gi


# ------------------------------------------------------------------ replaid.scse
SCSE_KINDS = ("signed", "nonneg")


@functools.lru_cache(maxsize=None)
def scse_case(kind, sparse):
    """(X, Gp, Gi): g = 1501, n = 37.  "signed": negatives and zeros (removeLog2 = NULL resolves FALSE); "nonneg": zeros,
    values below 20 (NULL resolves TRUE).  sparse: a scipy CSC matrix that also stores a few zeros (2^0 = 1 under
    removeLog2) and, when signed, its negatives"""
    g, n = 1501, 37
    rng = np.random.default_rng(len(kind) + 2 * int(sparse))
    X = np.minimum(rng.gamma(2.0, 1.5, size=(g, n)), 19.5)
    X[rng.random(X.shape) < (0.8 if sparse else 0.2)] = 0.0
    if kind == "signed":
        X *= np.where(rng.random(X.shape) < 0.3, -1.0, 1.0)
    assert X.min() <= 0.0 and X.max() < 20.0
    Gp, Gi = sets(g, 80, 77, kmin=1, kmax=300)
    if not sparse:
        return np.asfortranarray(X), Gp, Gi
    return _with_stored_zeros(X, [(r, c) for r, c in zip(*np.nonzero(X == 0.0))][:40]), Gp, Gi
