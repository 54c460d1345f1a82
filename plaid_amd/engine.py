"""Thin object layer over the C ABI: a device context, a prepared gene-set handle, and the
device-level / host-level calls.  Pointers are plain integers (`tensor.data_ptr()`,
`ndarray.ctypes.data`); no tensor types cross the boundary."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import STAT, TIES, check


def _np_ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _as_f64_fortran(a) -> np.ndarray:
    return np.asfortranarray(a, dtype=np.float64)


_INT32_MAX = 2**31 - 1


def _as_i32(a) -> np.ndarray:
    """dgCMatrix-style index arrays are 32-bit at the boundary (include/plaidhip.h).  scipy hands over int64
    for large matrices: refuse, instead of wrapping, anything a 32-bit slot cannot hold (more than 2^31-1
    stored values: split the matrix by columns first, as `chunked_crossprod` does, R/plaid.R:100-123)."""
    a = np.asarray(a)
    if a.dtype != np.int32 and a.size:
        lo, hi = int(a.min()), int(a.max())
        if lo < -_INT32_MAX - 1 or hi > _INT32_MAX:
            raise _lib.PlaidHipError(_lib.EUNSUPPORTED,
                                     f"index value {hi if hi > _INT32_MAX else lo} does not fit the 32-bit dgCMatrix slots of the "
                                     "C ABI (more than 2^31-1 stored values?): split the matrix by columns")
    return np.ascontiguousarray(a, dtype=np.int32)


class Geneset:
    """Device-resident prepared membership (plaidhip_geneset)."""

    def __init__(self, ctx: "Context", g: int, Gp, Gi):
        Gp = _as_i32(Gp)
        Gi = _as_i32(Gi)
        self.ctx = ctx
        self.g = int(g)
        self.m = int(len(Gp) - 1)
        self.sizes = np.diff(Gp).astype(np.int64)
        h = C.c_void_p()
        check(ctx.lib.plaidhip_geneset_create(ctx.handle, self.g, self.m, _np_ptr(Gp), _np_ptr(Gi), C.byref(h)))
        self.handle = h

    def info(self) -> dict:
        buf = (C.c_int64 * 8)()
        check(self.ctx.lib.plaidhip_geneset_info(self.handle, buf))
        return {"g": buf[0], "m": buf[1], "z": buf[2], "padded_slots": buf[3], "tiles": buf[4],
                "gene_slices": buf[5], "waves": buf[6], "padded_slots_pair": buf[7]}

    def close(self):
        if self.handle:
            self.ctx.lib.plaidhip_geneset_destroy(self.handle)
            self.handle = None

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass


def _x_args(X):
    """(Xp, Xi, values, g, n, keepalive) for a dense ndarray or a scipy CSC matrix."""
    if not isinstance(X, np.ndarray):
        import scipy.sparse as sp
        if sp.issparse(X):
            X = sp.csc_matrix(X)
            return _slots(X.indptr, X.indices, X.data, X.shape[0])
    Xd = _as_f64_fortran(X)
    return None, None, _np_ptr(Xd), Xd.shape[0], Xd.shape[1], (Xd,)


def _slots(Xp, Xi, Xx, g):
    """_x_args of the slots of a g x n CSC matrix"""
    Xp, Xi = _as_i32(Xp), _as_i32(Xi)
    Xx = np.ascontiguousarray(Xx, dtype=np.float64)
    return _np_ptr(Xp), _np_ptr(Xi), _np_ptr(Xx), int(g), len(Xp) - 1, (Xp, Xi, Xx)


def _result(out, m, n):
    """the caller's own result buffer (any byte offset; Fortran order like an R matrix) or a fresh one"""
    if out is None:
        return np.empty((m, n), dtype=np.float64, order="F")
    if out.shape != (m, n) or out.dtype != np.float64 or not out.flags.f_contiguous or not out.flags.writeable:
        raise ValueError(f"out: a writeable Fortran-ordered float64 array of shape {(m, n)}")
    return out


def _score(fn, head, X, Gp, Gi, *tail, pre=(), post=(), dense=False, out=None, cols=None):
    """The one marshaller of the host-level scorers: fn(*head, X, g, n, *pre, Gp, Gi, m, *tail, result, *post).  head: (handle,) of
    a context entry, (devices pointer, ndev) of a plaidhip_*_multi entry, (device, nshards, fail_shard) of a test hook; X: a
    dense array, a scipy CSC matrix or _slots(); dense: the entry takes no Xp / Xi.  The result is m x n, or m x cols."""
    xp, xi, xv, g, n, keep = X if isinstance(X, tuple) else _x_args(X)
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    m = len(Gp) - 1
    S = _result(out, m, n if cols is None else cols)
    x = (xv, g, n) if dense else (xp, xi, xv, g, n)
    check(fn(*head, *x, *pre, _np_ptr(Gp), _np_ptr(Gi), m, *tail, _np_ptr(S), *post))
    return S


def _rowtf(rowtf) -> int:
    if rowtf not in ("z", "ecdf"):
        raise ValueError("Error: unknown row transform" + str(rowtf))          # R/plaid.R:348
    return 0 if rowtf == "z" else 1


def _remove_log2(remove_log2) -> int:
    return -1 if remove_log2 is None else int(bool(remove_log2))


def _plaid_test(fn, head, X, y, Gp, Gi, gsetX, tests, metap_method, dense=False, out=None):
    """plaid.test through _score: sets x 6 (gsetFC, p.one, p.two, p.lm, p.meta, q.meta), G's column order"""
    X = X if isinstance(X, tuple) else _x_args(X)
    n, m = X[4], len(Gp) - 1
    y = np.ascontiguousarray(y, dtype=np.int32)
    if y.shape != (n,):
        raise ValueError("y must have one entry per column of X")
    sx = None
    if gsetX is not None:
        sx = _as_f64_fortran(gsetX)
        if sx.shape != (m, n):
            raise ValueError("gsetX must be sets x samples")
    return _score(fn, head, X, Gp, Gi, None if sx is None else _np_ptr(sx), int(tests), int(metap_method), pre=(_np_ptr(y),),
                  dense=dense, out=out, cols=6)


def contrast_labels(Y, n):
    """Y of plaid.test.contrasts as the C ABI takes it: n x C int32, Fortran order, -1 for NA.  Y: integers (0, 1, -1) or
    floats (0, 1, NaN or -1); one column may come as a vector.  Other values are kept (rounded towards zero, an out-of-range
    or fractional one as 2) for the library's own check to name."""
    Y = np.asarray(Y)
    if Y.ndim == 1:
        Y = Y[:, None]
    if Y.ndim != 2 or Y.shape[0] != n:
        raise ValueError("Y must have one row per column of X")
    if Y.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            bad = ~np.isnan(Y) & ~np.isin(Y, (0.0, 1.0, -1.0))
            Y = np.where(np.isnan(Y), -1.0, np.where(bad, 2.0, Y))
    elif Y.dtype.kind not in "iub":
        raise ValueError("Y must be numeric: 0, 1, and NaN or -1 for a sample that takes no part")
    else:
        Y = np.where((Y < -1) | (Y > 1), 2, Y)
    return np.asfortranarray(Y, dtype=np.int32)


def contrast_tile() -> int:
    """PLAIDHIP_CONTRAST_TILE: the contrasts that share one read of the matrix (needs no device)"""
    return int(_lib.load().plaidhip_contrast_tile())


def _plaid_test_contrasts(fn, head, X, Y, Gp, Gi, gsetX, tests, metap_method, dense=False, out=None):
    """plaid.test.contrasts through _score: sets x 6 x C, [:, :, j] what _plaid_test returns for contrast j"""
    X = X if isinstance(X, tuple) else _x_args(X)
    n, m = X[4], len(Gp) - 1
    Y = contrast_labels(Y, n)
    ncon = Y.shape[1]
    sx = None
    if gsetX is not None:
        sx = _as_f64_fortran(gsetX)
        if sx.shape != (m, n):
            raise ValueError("gsetX must be sets x samples")
    if out is None:
        out = np.empty((m, 6, ncon), dtype=np.float64, order="F")
    elif out.shape != (m, 6, ncon) or out.dtype != np.float64 or not out.flags.f_contiguous or not out.flags.writeable:
        raise ValueError(f"out: a writeable Fortran-ordered float64 array of shape {(m, 6, ncon)}")
    flat = out.reshape((m, 6 * ncon), order="F")   # (a view: contrast j's six columns are columns 6 j .. 6 j + 5)
    _score(fn, head, X, Gp, Gi, None if sx is None else _np_ptr(sx), int(tests), int(metap_method), pre=(_np_ptr(Y), ncon),
           dense=dense, out=flat, cols=6 * ncon)
    return out


GSVA_EXACT_ROWTF = {"z": 0, "ecdf": 1, "none": 2, "gauss": 3}
GSVA_KCDF_TABLE = 10001   # PLAIDHIP_GSVA_KCDF_TABLE


def check_gsva_exact_args(tau, rowtf):
    """the checks of plaidhip_gsva_exact that need no device: (tau, the row transform's code)"""
    rowtf = rowtf if isinstance(rowtf, str) else rowtf[0]
    tau = float(tau)
    if not np.isfinite(tau) or tau < 0.0:
        raise ValueError(f"gsva_exact: tau must be finite and >= 0 (got {tau:g})")
    if rowtf not in GSVA_EXACT_ROWTF:
        raise ValueError("Error: unknown row transform" + str(rowtf))          # R/plaid.R:348
    return tau, GSVA_EXACT_ROWTF[rowtf]


def _scse(fn, head, X, Gp, Gi, remove_log2, score_mean):
    """(S, whether the 2 ** x transform ran): the automatic decision is taken on the device (R/plaid.R:160-161)"""
    removed = C.c_int(0)
    S = _score(fn, head, X, Gp, Gi, _remove_log2(remove_log2), int(bool(score_mean)), post=(C.byref(removed),))
    return S, bool(removed.value)


def gsva_kcdf_table() -> np.ndarray:
    """the 10,001 values of Phi on [0, 10] that the kernels of gsva_kcdf read (built on the host: needs no device)"""
    T = np.empty(GSVA_KCDF_TABLE, dtype=np.float64)
    check(_lib.load().plaidhip_gsva_kcdf_table(_np_ptr(T)))
    return T


SING_EXACT_MAX_GENES = 131072   # PLAIDHIP_GSEA_KS_MAX_GENES: the dispersion kernel's bitmap
SING_EXACT_OUTPUTS = ("TotalScore", "UpScore", "DownScore", "TotalDispersion", "UpDispersion", "DownDispersion")


def check_sing_exact_args(g, Gp, Dp, dispersion):
    """the checks of plaidhip_sing_exact that need no device"""
    if Dp is not None and len(Dp) != len(Gp):
        raise ValueError(f"sing_exact: the down sets have {len(Dp) - 1} columns, the up sets {len(Gp) - 1}")
    if dispersion and g > SING_EXACT_MAX_GENES:
        raise _lib.PlaidHipError(_lib.EUNSUPPORTED,
                                 f"sing_exact: nrow(X) = {g} (at most {SING_EXACT_MAX_GENES} rows with the dispersion)")


def _sing_exact_call(fn, head, X, Gp, Gi, Dp, Di, center, dispersion, fill=None):
    """fill: what the results hold before the call (the tests' sentinel); None leaves them uninitialised"""
    xp, xi, xv, g, n, keep = _x_args(X)
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    down = Dp is not None
    if down:
        Dp, Di = _as_i32(Dp), _as_i32(Di)
    check_sing_exact_args(g, Gp, Dp if down else None, dispersion)
    m = len(Gp) - 1
    want = [down, True, down, down and dispersion, bool(dispersion), down and dispersion]
    outs = [(np.empty if fill is None else np.full)((m, n), *(() if fill is None else (fill,)), dtype=np.float64, order="F")
            if w else None for w in want]
    check(fn(*head, xp, xi, xv, g, n, _np_ptr(Gp), _np_ptr(Gi), _np_ptr(Dp) if down else None, _np_ptr(Di) if down else None, m,
             int(bool(center)), *[None if o is None else _np_ptr(o) for o in outs]))
    return {name: o for name, o in zip(SING_EXACT_OUTPUTS, outs) if o is not None}


UCELL_EXACT_OUTPUTS = ("TotalScore", "UpScore", "DownScore")
TRUNC_MODE = {"ucell": 0, "aucell": 1}   # PLAIDHIP_TRUNC_*


def check_truncated_rank(who, what, g, rank):
    """maxRank / aucMaxRank as plaidhip_ucell_exact / plaidhip_aucell_exact check it, which needs no device"""
    r = float(rank)
    if not (1.0 <= r <= float(g)) or r != np.floor(r):
        raise ValueError(f"{who}: {what} must be an integer in 1..nrow(X) = {g} (got {r:g})")
    if 2.0 * float(g) * r >= 2.0 ** 53:
        raise _lib.PlaidHipError(_lib.EUNSUPPORTED, f"{who}: 2 nrow(X) {what} = 2 x {g} x {r:.0f} does not stay below 2^53")
    return r


def _ucell_exact_call(fn, head, X, Gp, Gi, Dp, Di, max_rank, w_neg, k_full, k_full_down, fill=None):
    """fill: what the results hold before the call (the tests' sentinel); None leaves them uninitialised"""
    xp, xi, xv, g, n, keep = _x_args(X)
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    down = Dp is not None
    if down:
        Dp, Di = _as_i32(Dp), _as_i32(Di)
        if len(Dp) != len(Gp):
            raise ValueError(f"ucell_exact: the down sets have {len(Dp) - 1} columns, the up sets {len(Gp) - 1}")
    w_neg = float(w_neg)
    if not np.isfinite(w_neg) or w_neg < 0.0:
        raise ValueError(f"ucell_exact: w_neg must be finite and >= 0 (got {w_neg:g})")
    m = len(Gp) - 1
    impute = k_full is not None
    kf = np.ascontiguousarray(k_full, dtype=np.float64) if impute else None
    kd = np.ascontiguousarray(k_full_down, dtype=np.float64) if impute and k_full_down is not None else None
    if impute and (kf.shape != (m,) or (kd is not None and kd.shape != (m,))):
        raise ValueError("ucell_exact: k_full must have one entry per set")
    outs = [(np.empty if fill is None else np.full)((m, n), *(() if fill is None else (fill,)), dtype=np.float64, order="F")
            if w else None for w in (down, True, down)]
    check(fn(*head, xp, xi, xv, g, n, _np_ptr(Gp), _np_ptr(Gi), _np_ptr(Dp) if down else None, _np_ptr(Di) if down else None, m,
             float(max_rank), w_neg, int(impute), None if kf is None else _np_ptr(kf), None if kd is None else _np_ptr(kd),
             *[None if o is None else _np_ptr(o) for o in outs]))
    return {name: o for name, o in zip(UCELL_EXACT_OUTPUTS, outs) if o is not None}


GSEA_KS_MAX_GENES = 131072   # PLAIDHIP_GSEA_KS_MAX_GENES
GSEA_COLUMNS = ("ES", "NES", "pval", "padj", "nMoreExtreme", "size", "nGeEs", "nLeEs", "nGeZero", "nLeZero", "sumPos", "sumNeg")


def check_gsea_args(stat, weight, perm, nperm):
    """the checks of plaidhip_gsea that need no device, in its order: (stat, weight, perm or None, nperm) as the ABI takes
    them.  stat / weight: g genes x c lists (a vector is one list); perm: g x nperm int32 placements or None."""
    stat = _as_f64_fortran(stat)
    if stat.ndim == 1:
        stat = np.asfortranarray(stat.reshape(-1, 1))
    weight = _as_f64_fortran(weight)
    if weight.ndim == 1:
        weight = np.asfortranarray(weight.reshape(-1, 1))
    if stat.ndim != 2 or weight.shape != stat.shape:
        raise ValueError("gsea: stat and weight must be genes x lists of one shape")
    if perm is not None:
        perm = np.asfortranarray(perm, dtype=np.int32)
        if perm.ndim != 2 or perm.shape[0] != stat.shape[0]:
            raise ValueError("gsea: perm must be genes x permutations")
        nperm = perm.shape[1]
    nperm = int(nperm)
    if nperm < 1:
        raise ValueError(f"gsea: nperm = {nperm} (at least 1)")
    if stat.shape[1] < 1:
        raise ValueError("gsea: 0 ranked lists (at least 1)")
    if stat.shape[0] > GSEA_KS_MAX_GENES:
        raise _lib.PlaidHipError(_lib.EUNSUPPORTED, f"gsea: {stat.shape[0]} genes (at most {GSEA_KS_MAX_GENES})")
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(weight) & (weight >= 0.0))
    if bad.any():
        raise ValueError(f"gsea: weight[{int(np.flatnonzero(bad.ravel(order='F'))[0])}] is not finite and >= 0")
    return stat, weight, perm, nperm


GSEA_SCORE_TYPES = {"std": 0, "pos": 1, "neg": 2}   # PLAIDHIP_GSEA_STD / _POS / _NEG


def gsea_score_type(score_type):
    """the ABI's ordinal of a score type name (an ordinal passes through, so a test reaches the library's own check)"""
    if isinstance(score_type, str):
        if score_type not in GSEA_SCORE_TYPES:
            raise ValueError(f"gsea: score_type must be one of {sorted(GSEA_SCORE_TYPES)} (got {score_type!r})")
        return GSEA_SCORE_TYPES[score_type]
    return int(score_type)


def _gsea(fn, head, stat, weight, Gp, Gi, perm=None, nperm=1000, seed=1, null=False, score_type=None, leading_edge=False):
    """plaidhip_gsea / _multi / the hook: sets x 12 x lists (GSEA_COLUMNS), and the sets x nperm x lists null scores with
    null = True.  score_type not None: `fn` is plaidhip_gsea_scored / _multi / its hook; with leading_edge the result ends
    with le_len (sets x lists int32) and le_idx (Gp[-1] x lists int32, -1 past a set's edge)"""
    stat, weight, perm, nperm = check_gsea_args(stat, weight, perm, nperm)
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    g, c = stat.shape
    m = len(Gp) - 1
    out = np.full((m, 12, c), np.nan, dtype=np.float64, order="F")
    nul = np.full((m, nperm, c), np.nan, dtype=np.float64, order="F") if null else None
    tail = ()
    res = (out, nul) if null else (out,)
    if score_type is not None:
        le_len = np.full((m, c), -7, dtype=np.int32, order="F") if leading_edge else None
        le_idx = np.full((int(Gp[-1]), c), -7, dtype=np.int32, order="F") if leading_edge else None
        tail = (None if le_len is None else _np_ptr(le_len), None if le_idx is None else _np_ptr(le_idx))
        if leading_edge:
            res += (le_len, le_idx)
    check(fn(*head, _np_ptr(stat), _np_ptr(weight), g, c, _np_ptr(Gp), _np_ptr(Gi), m, None if perm is None else _np_ptr(perm),
             nperm, int(seed) & (2**64 - 1), *(() if score_type is None else (gsea_score_type(score_type),)), _np_ptr(out),
             None if nul is None else _np_ptr(nul), *tail))
    return res if len(res) > 1 else out


GSEA_ML_MAX_STAGES = 256     # PLAIDHIP_GSEA_ML_MAX_STAGES
GSEA_ML_MAX_SAMPLE = 1023    # PLAIDHIP_GSEA_ML_MAX_SAMPLE
GSEA_ML_COLUMNS = ("pvalML", "log2err", "stage", "status", "qhat", "denom")
GSEA_ML_STATUS = ("estimated", "floor", "stalled")   # PLAIDHIP_GSEA_ML_ESTIMATED / _FLOOR / _STALLED


def check_gsea_ml_args(who, sample_size, sweeps, eps):
    """the checks of the chains' own parameters, in the library's order"""
    sample_size, sweeps, eps = int(sample_size), int(sweeps), float(eps)
    if not (3 <= sample_size <= GSEA_ML_MAX_SAMPLE and sample_size % 2 == 1):
        raise ValueError(f"{who}: sample_size = {sample_size} (odd, 3..{GSEA_ML_MAX_SAMPLE})")
    if not 1 <= sweeps <= 32:
        raise ValueError(f"{who}: sweeps = {sweeps} (1..32)")
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"{who}: eps = {eps:g} (0 <= eps < 1)")
    return sample_size, sweeps, eps


def _gsea_multilevel(fn, head, stat, weight, Gp, Gi, perm=None, nperm=1000, seed=1, null=False, score_type="std",
                     leading_edge=False, sample_size=101, sweeps=4, eps=1e-50, ml_min=10):
    """plaidhip_gsea_multilevel / _multi / the hook: (out, ml[, null][, le_len, le_idx]) -- out as _gsea's with the reported
    pval and padj, ml sets x 6 x lists (GSEA_ML_COLUMNS; NaN for a pair without a ruler)"""
    sample_size, sweeps, eps = check_gsea_ml_args("gsea_multilevel", sample_size, sweeps, eps)
    ml_min = int(ml_min)
    if ml_min < 0:
        raise ValueError(f"gsea_multilevel: ml_min = {ml_min} (at least 0)")
    stat, weight, perm, nperm = check_gsea_args(stat, weight, perm, nperm)
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    g, c = stat.shape
    m = len(Gp) - 1
    out = np.full((m, 12, c), np.nan, dtype=np.float64, order="F")
    ml = np.full((m, 6, c), np.nan, dtype=np.float64, order="F")
    nul = np.full((m, nperm, c), np.nan, dtype=np.float64, order="F") if null else None
    le_len = np.full((m, c), -7, dtype=np.int32, order="F") if leading_edge else None
    le_idx = np.full((int(Gp[-1]), c), -7, dtype=np.int32, order="F") if leading_edge else None
    check(fn(*head, _np_ptr(stat), _np_ptr(weight), g, c, _np_ptr(Gp), _np_ptr(Gi), m, None if perm is None else _np_ptr(perm),
             nperm, int(seed) & (2**64 - 1), gsea_score_type(score_type), sample_size, sweeps, eps, ml_min, _np_ptr(out),
             None if nul is None else _np_ptr(nul), None if le_len is None else _np_ptr(le_len),
             None if le_idx is None else _np_ptr(le_idx), _np_ptr(ml)))
    return (out, ml) + ((nul,) if null else ()) + ((le_len, le_idx) if leading_edge else ())


FISHER_MAX_GENES = 1 << 26   # PLAIDHIP_FISHER_MAX_GENES
FISHER_COLUMNS = ("size", "ovUp", "ovDn", "pUp", "pDn", "pAny", "padjUp", "padjDn", "padjAny", "orUp", "orDn", "orAny")


def check_fisher_args(sig):
    """the checks of plaidhip_fisher on sig that need no device, in its order: sig as the ABI takes it, g genes x c lists
    int8 of -1 / 0 / +1 (a vector is one list).  Values that are no integers in -1..1 (NaN among them) are refused here:
    an int8 cannot hold them."""
    a = np.asarray(sig)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2:
        raise ValueError("fisher: sig must be genes x lists")
    if a.shape[1] < 1:
        raise ValueError("fisher: 0 lists (at least 1)")
    if a.shape[0] > FISHER_MAX_GENES:
        raise _lib.PlaidHipError(_lib.EUNSUPPORTED, f"fisher: {a.shape[0]} genes (at most {FISHER_MAX_GENES})")
    if a.dtype != np.int8:
        bad = ~np.isin(a, (-1, 0, 1))
        if bad.any():
            e = int(np.flatnonzero(bad.ravel(order="F"))[0])
            raise ValueError(f"fisher: sig[{e}] = {a.ravel(order='F')[e]} (-1 down, 0, +1 up)")
    return np.asfortranarray(a, dtype=np.int8)


def _fisher(fn, head, sig, Gp, Gi, overlap=False):
    """plaidhip_fisher / _multi / the hook: (out, tot) -- sets x 12 x lists (FISHER_COLUMNS) and the 2 x lists totals (nUp,
    nDn) -- and with overlap also ov_len (sets x lists int32) and ov_idx (Gp[-1] x lists int32, -1 past a set's overlap)"""
    sig = check_fisher_args(sig)
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    g, c = sig.shape
    m = len(Gp) - 1
    out = np.full((m, 12, c), np.nan, dtype=np.float64, order="F")
    tot = np.full((2, c), np.nan, dtype=np.float64, order="F")
    ov_len = np.full((m, c), -7, dtype=np.int32, order="F") if overlap else None
    ov_idx = np.full((int(Gp[-1]), c), -7, dtype=np.int32, order="F") if overlap else None
    check(fn(*head, _np_ptr(sig), g, c, _np_ptr(Gp), _np_ptr(Gi), m, _np_ptr(out), _np_ptr(tot),
             None if ov_len is None else _np_ptr(ov_len), None if ov_idx is None else _np_ptr(ov_idx)))
    return (out, tot, ov_len, ov_idx) if overlap else (out, tot)


def hyper_tail(N, K, k, x) -> float:
    """plaidhip_hyper_tail: P(X >= x), X ~ Hypergeometric(N, K, k), by the form pinned in include/plaidhip.h, on the host
    (no device is touched)"""
    p = C.c_double(np.nan)
    check(_lib.load().plaidhip_hyper_tail(int(N), int(K), int(k), int(x), C.byref(p)))
    return p.value


RANKCOR_MAX_GENES = 131072   # PLAIDHIP_RANKCOR_MAX_GENES
RANKCOR_COLUMNS = ("size", "rho", "t", "p.value", "q.value")
RANKCOR_TIES = {"average": 0, "min": 1, "max": 2}   # PLAIDHIP_TIES_AVERAGE / _MIN / _MAX


def rankcor_ties(ties):
    """the ABI's ordinal of a ties method name (an ordinal passes through, so a test reaches the library's own check);
    "random", the reference's method, is no function of the input and is refused"""
    if isinstance(ties, str):
        if ties not in RANKCOR_TIES:
            raise ValueError(f"rankcor: ties must be one of {sorted(RANKCOR_TIES)} (got {ties!r})")
        return RANKCOR_TIES[ties]
    return int(ties)


def check_rankcor_args(stat, use_rank=True, ties="average"):
    """the checks of plaidhip_rankcor that need no device, in its order: (stat, use_rank, ties) as the ABI takes them.
    stat: g genes x c lists of float64 (a vector is one list); NaN: the gene takes no part in that list"""
    a = _as_f64_fortran(stat)
    if a.ndim == 1:
        a = np.asfortranarray(a.reshape(-1, 1))
    if a.ndim != 2:
        raise ValueError("rankcor: stat must be genes x lists")
    if a.shape[1] < 1:
        raise ValueError("rankcor: 0 lists (at least 1)")
    t = rankcor_ties(ties)
    if a.shape[0] > RANKCOR_MAX_GENES:
        raise _lib.PlaidHipError(_lib.EUNSUPPORTED, f"rankcor: {a.shape[0]} genes (at most {RANKCOR_MAX_GENES})")
    return a, int(bool(use_rank)), t


def _rankcor(fn, head, stat, Gp, Gi, use_rank=True, ties="average"):
    """plaidhip_rankcor / _multi / the hook: (out, tot) -- sets x 5 x lists (RANKCOR_COLUMNS) and the lists' universe sizes"""
    stat, use_rank, ties = check_rankcor_args(stat, use_rank, ties)
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    g, c = stat.shape
    m = len(Gp) - 1
    out = np.full((m, 5, c), np.nan, dtype=np.float64, order="F")
    tot = np.full(c, np.nan, dtype=np.float64)
    check(fn(*head, _np_ptr(stat), g, c, _np_ptr(Gp), _np_ptr(Gi), m, use_rank, ties, _np_ptr(out), _np_ptr(tot)))
    return out, tot


def rankcor_finish(n, T1, T2, k, A) -> np.ndarray:
    """plaidhip_rankcor_finish: the rank-mode epilogue and Benjamini-Hochberg on integer operands, on the host (no device is
    touched).  n, T1, T2: one per list; k, A: sets x lists.  Returns sets x 5 x lists (RANKCOR_COLUMNS)"""
    n, T1, T2 = (np.ascontiguousarray(np.atleast_1d(v), dtype=np.int64) for v in (n, T1, T2))
    k, A = (np.asfortranarray(np.asarray(v, dtype=np.int64).reshape(-1, len(n))) for v in (k, A))
    m, c = k.shape
    if not (T1.shape == T2.shape == n.shape and A.shape == k.shape):
        raise ValueError("rankcor_finish: n, T1, T2 have one entry per list; k and A are sets x lists")
    out = np.full((m, 5, c), np.nan, dtype=np.float64, order="F")
    check(_lib.load().plaidhip_rankcor_finish(m, c, _np_ptr(n), _np_ptr(T1), _np_ptr(T2), _np_ptr(k), _np_ptr(A), _np_ptr(out)))
    return out


PLAGE_MAX_SET = 4096   # PLAIDHIP_PLAGE_MAX_SET
PLAGE_COLUMNS = ("size", "lambda", "explained", "iterations", "residual", "converged")
PLAGE_TOL = 2.0 ** -40


def _plage(fn, head, X, Gp, Gi, tol=PLAGE_TOL, maxit=1000, loadings=False, csc=None):
    """plaidhip_plage / _csc / _multi / the hook: (S, info[, loadings]) -- sets x samples, sets x 6 (PLAGE_COLUMNS) and the
    Gp[m] loadings in the sets' own segments of G.  csc: the entry takes the slots (True), a dense X alone (False), or
    either (None: the _multi form)"""
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    m = len(Gp) - 1
    info = np.full((m, 6), np.nan, dtype=np.float64, order="F")
    L = np.full(int(Gp[-1]), np.nan, dtype=np.float64) if loadings else None
    S = _score(fn, head, X, Gp, Gi, float(tol), int(maxit), post=(_np_ptr(info), None if L is None else _np_ptr(L)),
               dense=csc is False)
    return (S, info, L) if loadings else (S, info)


def _zscore(fn, head, X, Gp, Gi, csc=None):
    """plaidhip_zscore / _csc / _multi / the hook: (S, size) -- sets x samples and the sets' effective sizes"""
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    size = np.full(len(Gp) - 1, np.nan, dtype=np.float64)
    S = _score(fn, head, X, Gp, Gi, post=(_np_ptr(size),), dense=csc is False)
    return S, size


def _is_sparse(X):
    """whether _x_args would hand the entry the slots of a CSC matrix (a scipy sparse matrix, or _slots())"""
    if isinstance(X, tuple):
        return X[0] is not None
    return not isinstance(X, np.ndarray) and hasattr(X, "tocsc")


LIMMA_MAX_COEF = 32   # PLAIDHIP_LIMMA_MAX_COEF
LIMMA_COLUMNS = ("logFC", "AveExpr", "t", "P.Value", "adj.P.Val", "sigma2")
LIMMA_HYPER = ("df.residual", "df.prior", "s2.prior", "n.ok")
LIMMA_NA_MAX_COEF = 10   # PLAIDHIP_LIMMA_NA_MAX_COEF
LIMMA_HYPER_NA = LIMMA_HYPER + ("df.pooled",)
LIMMA_NA = ("propagate", "fit")


def limma_tile() -> int:
    """PLAIDHIP_LIMMA_TILE: the weight columns that share one read of the matrix (needs no device)"""
    return int(_lib.load().plaidhip_limma_tile())


def limma_operands(n, design, use=None, contrasts=None):
    """design, use and contrasts as the C ABI takes them: (D n x p x nfit float64, use n x nfit int8 or None, K p x q float64
    or None, q), all Fortran-ordered.  design: n x p (one fit) or n x p x nfit; use: n or n x nfit, anything that is zero,
    False or NaN leaves the sample out; contrasts: p or p x q."""
    D = np.asarray(design, dtype=np.float64)
    if D.ndim == 2:
        D = D[:, :, None]
    if D.ndim != 3 or D.shape[0] != n:
        raise ValueError("design must be samples x coefficients (x fits), one row per column of the matrix")
    D = np.asfortranarray(D)
    p, nfit = D.shape[1], D.shape[2]
    U = None
    if use is not None:
        U = np.asarray(use)
        if U.ndim == 1:
            U = U[:, None]
        if U.shape != (n, nfit):
            raise ValueError("use must be samples x fits")
        if U.dtype.kind == "f":
            U = ~np.isnan(U) & (U != 0)
        U = np.asfortranarray(U != 0, dtype=np.int8)
    K = None
    if contrasts is not None:
        K = np.asarray(contrasts, dtype=np.float64)
        if K.ndim == 1:
            K = K[:, None]
        if K.ndim != 2 or K.shape[0] != p:
            raise ValueError("contrasts must be coefficients x contrasts")
        K = np.asfortranarray(K)
    return D, U, K, (p if K is None else K.shape[1])


def _limma(fn, head, A, design, use=None, contrasts=None, out=None, hyper=None):
    """plaidhip_limma / _multi / the hook: (out, hyper) -- rows x 6 x q x nfit (LIMMA_COLUMNS) and nfit x 4 (LIMMA_HYPER)"""
    A = _as_f64_fortran(A)
    if A.ndim != 2:
        raise ValueError("limma: the matrix must be rows x samples")
    rows, n = A.shape
    D, U, K, q = limma_operands(n, design, use, contrasts)
    p, nfit = D.shape[1], D.shape[2]
    out = np.full((rows, 6, q, nfit), np.nan, dtype=np.float64, order="F") if out is None else out
    hyper = np.full((nfit, 4), np.nan, dtype=np.float64) if hyper is None else hyper
    check(fn(*head, _np_ptr(A), rows, n, _np_ptr(D), p, nfit, None if U is None else _np_ptr(U), None if K is None else _np_ptr(K),
             q, _np_ptr(out), _np_ptr(hyper)))
    return out, hyper


def _limma_na(fn, head, A, design, use=None, contrasts=None, max_na=0.2, out=None, hyper=None, dfres=None):
    """plaidhip_limma_na / _multi / the hook (na = "fit"): (out, hyper, dfres) -- rows x 6 x q x nfit, nfit x 5
    (LIMMA_HYPER_NA) and rows x nfit, the df.residual of every fitted (row, fit), NaN for the others"""
    A = _as_f64_fortran(A)
    if A.ndim != 2:
        raise ValueError("limma: the matrix must be rows x samples")
    rows, n = A.shape
    D, U, K, q = limma_operands(n, design, use, contrasts)
    p, nfit = D.shape[1], D.shape[2]
    out = np.full((rows, 6, q, nfit), np.nan, dtype=np.float64, order="F") if out is None else out
    hyper = np.full((nfit, 5), np.nan, dtype=np.float64) if hyper is None else hyper
    dfres = np.full((rows, nfit), np.nan, dtype=np.float64, order="F") if dfres is None else dfres
    check(fn(*head, _np_ptr(A), rows, n, _np_ptr(D), p, nfit, None if U is None else _np_ptr(U), None if K is None else _np_ptr(K),
             q, float(max_na), _np_ptr(out), _np_ptr(hyper), _np_ptr(dfres)))
    return out, hyper, dfres


def limma_weights(rows, n, weights):
    """weights as the C ABI takes them: (Wt rows x n float64 Fortran-ordered or None, aw n float64 or None).  weights: a rows x
    n matrix (observation weights), a vector of n (array weights), or a pair (matrix, vector)"""
    if isinstance(weights, tuple):
        Wt, aw = weights
    else:
        w = np.asarray(weights, dtype=np.float64)
        Wt, aw = (None, w) if w.ndim == 1 else (w, None)
    if Wt is not None:
        Wt = _as_f64_fortran(np.asarray(Wt, dtype=np.float64))
        if Wt.shape != (rows, n):
            raise ValueError("limma: observation weights must have the shape of the matrix, rows x samples")
    if aw is not None:
        aw = np.ascontiguousarray(np.asarray(aw, dtype=np.float64))
        if aw.shape != (n,):
            raise ValueError("limma: array weights must have one entry per sample")
    return Wt, aw


def _limma_w(fn, head, A, weights, design, use=None, contrasts=None, max_na=0.2, out=None, hyper=None, dfres=None):
    """plaidhip_limma_w / _multi / the hook (weights): (out, hyper, dfres) as _limma_na returns them"""
    A = _as_f64_fortran(A)
    if A.ndim != 2:
        raise ValueError("limma: the matrix must be rows x samples")
    rows, n = A.shape
    Wt, aw = limma_weights(rows, n, weights)
    D, U, K, q = limma_operands(n, design, use, contrasts)
    p, nfit = D.shape[1], D.shape[2]
    out = np.full((rows, 6, q, nfit), np.nan, dtype=np.float64, order="F") if out is None else out
    hyper = np.full((nfit, 5), np.nan, dtype=np.float64) if hyper is None else hyper
    dfres = np.full((rows, nfit), np.nan, dtype=np.float64, order="F") if dfres is None else dfres
    check(fn(*head, _np_ptr(A), None if Wt is None else _np_ptr(Wt), None if aw is None else _np_ptr(aw), rows, n, _np_ptr(D), p,
             nfit, None if U is None else _np_ptr(U), None if K is None else _np_ptr(K), q, float(max_na), _np_ptr(out),
             _np_ptr(hyper), _np_ptr(dfres)))
    return out, hyper, dfres


def _limma_any(fn, fn_na, head, A, design, use, contrasts, na, max_na, weights=None, fn_w=None):
    if na not in LIMMA_NA:
        raise ValueError(f"limma: na must be one of {LIMMA_NA}")
    if weights is not None:   # (limma's rule: a NaN or a weight that is not positive and finite is a missing observation)
        return _limma_w(fn_w, head, A, weights, design, use, contrasts, max_na if na == "fit" else 0.0)
    if na == "fit":
        return _limma_na(fn_na, head, A, design, use, contrasts, max_na)
    return _limma(fn, head, A, design, use, contrasts)


def limma_na_solve(qmis, Ep, nobs, v) -> dict:
    """plaidhip_limma_na_solve on the host (no device is touched): the refit of one incomplete row.  qmis: nmis x p, the rows
    of Q_f of its missing samples in ascending order; Ep: E' (p); nobs: its observed samples; v: p x q -> gamma (p), u (q),
    the Cholesky pivots (p) and ok"""
    qmis = np.ascontiguousarray(np.asarray(qmis, dtype=np.float64))
    Ep = np.ascontiguousarray(np.asarray(Ep, dtype=np.float64))
    p = Ep.shape[0]
    qmis = qmis.reshape(-1, p)
    v = np.asfortranarray(np.asarray(v, dtype=np.float64).reshape(p, -1))
    q = v.shape[1]
    gamma, u, piv = np.full(p, -7.0), np.full(q, -7.0), np.full(p, -7.0)
    ok = C.c_int32(-7)
    check(_lib.load().plaidhip_limma_na_solve(p, qmis.shape[0], _np_ptr(qmis), _np_ptr(Ep), int(nobs), _np_ptr(v), q,
                                              _np_ptr(gamma), _np_ptr(u), _np_ptr(piv), C.cast(C.byref(ok), C.c_void_p)))
    return {"gamma": gamma, "u": u, "pivots": piv, "ok": bool(ok.value)}


VOOM_MAX_KNOTS = 256


def _voom(fn, head, counts, design, lib_size=None, span=0.5, out=None):
    """plaidhip_voom / _multi / the hook: dict of E and weights (rows x samples), lib_size and offset (samples), knots_x and
    knots_y (the trend's knots).  out: a dict of caller's buffers E, W, lib, off, kx, ky (the tests' sentinels)"""
    A = _as_f64_fortran(counts)
    if A.ndim != 2:
        raise ValueError("voom: counts must be rows x samples")
    rows, n = A.shape
    D = np.asfortranarray(np.asarray(design, dtype=np.float64))
    if D.ndim != 2 or D.shape[0] != n:
        raise ValueError("voom: design must be samples x coefficients, one row per column of counts")
    L = None
    if lib_size is not None:
        L = np.ascontiguousarray(np.asarray(lib_size, dtype=np.float64))
        if L.shape != (n,):
            raise ValueError("voom: lib_size must have one entry per sample")
    o = out if out is not None else {}
    E = o.get("E", np.full((rows, n), np.nan, order="F"))
    W = o.get("W", np.full((rows, n), np.nan, order="F"))
    lib, off = o.get("lib", np.full(n, np.nan)), o.get("off", np.full(n, np.nan))
    kx, ky = o.get("kx", np.full(VOOM_MAX_KNOTS, np.nan)), o.get("ky", np.full(VOOM_MAX_KNOTS, np.nan))
    nk = C.c_int32(0)
    check(fn(*head, _np_ptr(A), rows, n, _np_ptr(D), D.shape[1], None if L is None else _np_ptr(L), float(span), _np_ptr(E),
             _np_ptr(W), _np_ptr(lib), _np_ptr(off), _np_ptr(kx), _np_ptr(ky), C.cast(C.byref(nk), C.c_void_p)))
    return {"E": E, "weights": W, "lib_size": lib, "offset": off, "knots_x": kx[:nk.value].copy(), "knots_y": ky[:nk.value].copy()}


def lowess(x, y, f=2.0 / 3.0, iter=3, delta=None) -> dict:
    """plaidhip_lowess on the host (no device is touched): R's lowess as pinned in include/plaidhip.h.  x ascending.  Returns
    ys (the fitted values) and anchor (bool: where the last pass made a local fit or a tie copy)"""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("lowess: x and y are vectors of one length")
    if delta is None:
        delta = 0.01 * (x[-1] - x[0]) if len(x) else 0.0
    ys, anchor = np.full(len(x), np.nan), np.zeros(len(x), dtype=np.int8)
    check(_lib.load().plaidhip_lowess(_np_ptr(x), _np_ptr(y), len(x), float(f), int(iter), float(delta), _np_ptr(ys),
                                      _np_ptr(anchor)))
    return {"ys": ys, "anchor": anchor != 0}


def limma_w_solve(Htri, b, nlive, v) -> dict:
    """plaidhip_limma_w_solve on the host (no device is touched): the weighted fit of one row from its sums.  Htri: the lower
    triangle of H row by row (p (p + 1) / 2); b (p); nlive: its live observations; v: p x q -> gamma (p), u (q), the Cholesky
    pivots (p) and ok"""
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
    p = b.shape[0]
    Htri = np.ascontiguousarray(np.asarray(Htri, dtype=np.float64))
    if Htri.shape != (p * (p + 1) // 2,):
        raise ValueError("limma_w_solve: Htri holds the p (p + 1) / 2 entries of the lower triangle")
    v = np.asfortranarray(np.asarray(v, dtype=np.float64).reshape(p, -1))
    q = v.shape[1]
    gamma, u, piv = np.full(p, -7.0), np.full(q, -7.0), np.full(p, -7.0)
    ok = C.c_int32(-7)
    check(_lib.load().plaidhip_limma_w_solve(p, _np_ptr(Htri), _np_ptr(b), int(nlive), _np_ptr(v), q, _np_ptr(gamma), _np_ptr(u),
                                             _np_ptr(piv), C.cast(C.byref(ok), C.c_void_p)))
    return {"gamma": gamma, "u": u, "pivots": piv, "ok": bool(ok.value)}


def limma_finish_na(E, rss, nf, v, drow, urow):
    """plaidhip_limma_finish_na on the host: limma_finish with the rows' own df.residual drow (nfit x rows, NaN: not fitted)
    and u (nfit q x rows) -> (out rows x 6 x q x nfit, hyper nfit x 5)"""
    v = np.asarray(v, dtype=np.float64)
    v = v[:, :, None] if v.ndim == 2 else v
    p, q, nfit = v.shape
    E = np.ascontiguousarray(np.asarray(E, dtype=np.float64).reshape(nfit * (p + 1), -1))
    rows = E.shape[1]
    rss = np.ascontiguousarray(np.asarray(rss, dtype=np.float64).reshape(nfit, rows))
    drow = np.ascontiguousarray(np.asarray(drow, dtype=np.float64).reshape(nfit, rows))
    urow = np.ascontiguousarray(np.asarray(urow, dtype=np.float64).reshape(nfit * q, rows))
    nf = np.ascontiguousarray(np.atleast_1d(nf), dtype=np.int64)
    v = np.asfortranarray(v)
    if nf.shape != (nfit,):
        raise ValueError("limma_finish_na: nf has one entry per fit")
    out = np.full((rows, 6, q, nfit), np.nan, dtype=np.float64, order="F")
    hyper = np.full((nfit, 5), np.nan, dtype=np.float64)
    check(_lib.load().plaidhip_limma_finish_na(rows, p, nfit, q, _np_ptr(E), _np_ptr(rss), _np_ptr(nf), _np_ptr(v), _np_ptr(drow),
                                               _np_ptr(urow), _np_ptr(out), _np_ptr(hyper)))
    return out, hyper


def limma_design(design, use=None, contrasts=None, fit=1) -> dict:
    """plaidhip_limma_design on the host (no device is touched): the thin Q (n x p, zero rows for the samples left out) and R
    of the Householder QR of one design's used rows, v = R^-T K (p x q), u = |v_j| (limma's stdev.unscaled) and n_f"""
    D0 = np.asarray(design, dtype=np.float64)
    if D0.ndim != 2:
        raise ValueError("limma_design: one design, samples x coefficients")
    D, U, K, q = limma_operands(D0.shape[0], D0, use, contrasts)
    n, p = D.shape[0], D.shape[1]
    Q = np.full((n, p), np.nan, order="F")
    R = np.full((p, p), np.nan, order="F")
    v = np.full((p, q), np.nan, order="F")
    u = np.full(q, np.nan)
    nf = C.c_int64(-1)
    check(_lib.load().plaidhip_limma_design(_np_ptr(D), n, p, None if U is None else _np_ptr(U), None if K is None else _np_ptr(K),
                                            q, int(fit), _np_ptr(Q), _np_ptr(R), _np_ptr(v), _np_ptr(u),
                                            C.cast(C.byref(nf), C.c_void_p)))
    return {"Q": Q, "R": R, "v": v, "u": u, "nf": int(nf.value)}


def limma_finish(E, rss, nf, v, u):
    """plaidhip_limma_finish on the host (no device is touched): E (nfit (p + 1)) x rows -- per fit its p effects, then the
    means --, rss nfit x rows, nf the samples of every fit, v p x q x nfit, u q x nfit -> (out rows x 6 x q x nfit, hyper
    nfit x 4)"""
    v = np.asarray(v, dtype=np.float64)
    v = v[:, :, None] if v.ndim == 2 else v
    p, q, nfit = v.shape
    E = np.ascontiguousarray(np.asarray(E, dtype=np.float64).reshape(nfit * (p + 1), -1))
    rows = E.shape[1]
    rss = np.ascontiguousarray(np.asarray(rss, dtype=np.float64).reshape(nfit, rows))
    nf = np.ascontiguousarray(np.atleast_1d(nf), dtype=np.int64)
    u = np.asfortranarray(np.asarray(u, dtype=np.float64).reshape((q, nfit), order="F"))
    v = np.asfortranarray(v)
    if nf.shape != (nfit,):
        raise ValueError("limma_finish: nf has one entry per fit")
    out = np.full((rows, 6, q, nfit), np.nan, dtype=np.float64, order="F")
    hyper = np.full((nfit, 4), np.nan, dtype=np.float64)
    check(_lib.load().plaidhip_limma_finish(rows, p, nfit, q, _np_ptr(E), _np_ptr(rss), _np_ptr(nf), _np_ptr(v), _np_ptr(u),
                                            _np_ptr(out), _np_ptr(hyper)))
    return out, hyper


CAMERA_COLUMNS = ("NGenes", "Correlation", "VIF", "t", "Down", "Up", "PValue", "FDR")
CAMERA_HYPER = LIMMA_HYPER + ("n.genes", "df.camera")


def check_camera_cor(inter_gene_cor):
    """inter_gene_cor as the C ABI takes it: a correlation inside (-1, 1), or None / NaN to estimate it from the residuals"""
    rho = np.nan if inter_gene_cor is None else float(inter_gene_cor)
    if not (np.isnan(rho) or -1.0 < rho < 1.0):
        raise ValueError(f"camera: inter_gene_cor = {rho:g} (a correlation inside (-1, 1), or None to estimate it)")
    return rho


def _camera(fn, head, X, design, Gp, Gi, use=None, contrasts=None, inter_gene_cor=0.01, allow_neg_cor=False, out=None,
            hyper=None):
    """plaidhip_camera / _multi / the hook: (out, hyper) -- sets x 8 x q x nfit (CAMERA_COLUMNS) and nfit x 6 (CAMERA_HYPER)"""
    X = _as_f64_fortran(X)
    if X.ndim != 2:
        raise ValueError("camera: the matrix must be genes x samples")
    g, n = X.shape
    D, U, K, q = limma_operands(n, design, use, contrasts)
    p, nfit = D.shape[1], D.shape[2]
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    m = len(Gp) - 1
    out = np.full((m, 8, q, nfit), np.nan, dtype=np.float64, order="F") if out is None else out
    hyper = np.full((nfit, 6), np.nan, dtype=np.float64) if hyper is None else hyper
    check(fn(*head, _np_ptr(X), g, n, _np_ptr(D), p, nfit, None if U is None else _np_ptr(U), None if K is None else _np_ptr(K),
             q, _np_ptr(Gp), _np_ptr(Gi), m, check_camera_cor(inter_gene_cor), int(bool(allow_neg_cor)), _np_ptr(out),
             _np_ptr(hyper)))
    return out, hyper


def camera_residual_row(x, Q, use, E, rss, d) -> np.ndarray:
    """plaidhip_camera_residual_row on the host (no device is touched): the standardised residuals of one gene.  x: n; Q: n x p,
    the fit's thin Q; use: n or None; E: the gene's p effects; rss and d = n_f - p"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(len(x), -1))
    E = np.ascontiguousarray(E, dtype=np.float64)
    U = None if use is None else np.ascontiguousarray(np.asarray(use) != 0, dtype=np.int8)
    z = np.full(len(x), -7.0)
    check(_lib.load().plaidhip_camera_residual_row(len(x), Q.shape[1], _np_ptr(x), _np_ptr(Q), None if U is None else _np_ptr(U),
                                                   _np_ptr(E), float(rss), float(d), _np_ptr(z)))
    return z


def camera_finish(t, ok, sumt, cnt, ss, dfres, dfprior, inter_gene_cor=None, allow_neg_cor=False):
    """plaidhip_camera_finish on the host (no device is touched): t genes x q x nfit, ok genes x nfit, sumt sets x q x nfit,
    cnt sets x nfit, ss sets x nfit (None: the fixed inter_gene_cor), dfres / dfprior per fit -> (out sets x 8 x q x nfit,
    gdf nfit x 2: the universe's size and df.camera)"""
    t = np.asarray(t, dtype=np.float64)
    t = np.asfortranarray(t[:, :, None] if t.ndim == 2 else t)
    g, q, nfit = t.shape
    ok = np.asfortranarray(np.asarray(ok).reshape((g, nfit), order="F") != 0, dtype=np.int8)
    cnt = np.asfortranarray(np.asarray(cnt, dtype=np.float64).reshape((-1, nfit), order="F"))
    m = cnt.shape[0]
    sumt = np.asfortranarray(np.asarray(sumt, dtype=np.float64).reshape((m, q, nfit), order="F"))
    ss = None if ss is None else np.asfortranarray(np.asarray(ss, dtype=np.float64).reshape((m, nfit), order="F"))
    dfres, dfprior = (np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64) for v in (dfres, dfprior))
    if dfres.shape != (nfit,) or dfprior.shape != (nfit,):
        raise ValueError("camera_finish: dfres and dfprior have one entry per fit")
    out = np.full((m, 8, q, nfit), -7.0, order="F")
    gdf = np.full((nfit, 2), -7.0)
    rho = np.nan if inter_gene_cor is None else float(inter_gene_cor)
    check(_lib.load().plaidhip_camera_finish(g, m, nfit, q, _np_ptr(t), _np_ptr(ok), _np_ptr(sumt), _np_ptr(cnt),
                                             None if ss is None else _np_ptr(ss), _np_ptr(dfres), _np_ptr(dfprior), rho,
                                             int(bool(allow_neg_cor)), _np_ptr(out), _np_ptr(gdf)))
    return out, gdf


FRY_COLUMNS = ("NGenes", "Direction", "t", "PValue", "FDR", "PValue.Mixed", "FDR.Mixed")
FRY_HYPER = LIMMA_HYPER + ("n.genes", "n.effects", "mixed")
FRY_STANDARDIZE = {"posterior.sd": 0, "residual.sd": 1, "none": 2}
FRY_MIXED_MAX = 128


def check_fry_standardize(standardize):
    """standardize as the C ABI takes it"""
    if standardize not in FRY_STANDARDIZE:
        raise ValueError(f"fry: standardize must be one of {sorted(FRY_STANDARDIZE)} (\"p2\" is not offered)")
    return FRY_STANDARDIZE[standardize]


def _fry(fn, head, X, design, Gp, Gi, use=None, contrasts=None, standardize="posterior.sd", out=None, hyper=None):
    """plaidhip_fry / _multi / the hook: (out, hyper) -- sets x 7 x q x nfit (FRY_COLUMNS) and nfit x 7 (FRY_HYPER)"""
    X = _as_f64_fortran(X)
    if X.ndim != 2:
        raise ValueError("fry: the matrix must be genes x samples")
    g, n = X.shape
    D, U, K, q = limma_operands(n, design, use, contrasts)
    p, nfit = D.shape[1], D.shape[2]
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    m = len(Gp) - 1
    out = np.full((m, 7, q, nfit), np.nan, dtype=np.float64, order="F") if out is None else out
    hyper = np.full((nfit, 7), np.nan, dtype=np.float64) if hyper is None else hyper
    check(fn(*head, _np_ptr(X), g, n, _np_ptr(D), p, nfit, None if U is None else _np_ptr(U), None if K is None else _np_ptr(K),
             q, _np_ptr(Gp), _np_ptr(Gi), m, check_fry_standardize(standardize), _np_ptr(out), _np_ptr(hyper)))
    return out, hyper


def fry_q2(design, use=None, fit=1) -> np.ndarray:
    """plaidhip_fry_q2 on the host (no device is touched): the n x (n_f - p) other columns of the full Householder Q of one
    design, the rows of the samples left out zero"""
    D0 = np.asarray(design, dtype=np.float64)
    if D0.ndim != 2:
        raise ValueError("fry_q2: one design, samples x coefficients")
    D, U, _, _ = limma_operands(D0.shape[0], D0, use, None)
    n, p = D.shape[0], D.shape[1]
    nf = n if U is None else int(U.sum())
    Q2 = np.full((n, max(nf - p, 0)), np.nan, order="F")
    got = C.c_int64(-1)
    check(_lib.load().plaidhip_fry_q2(_np_ptr(D), n, p, None if U is None else _np_ptr(U), int(fit), _np_ptr(Q2),
                                      C.cast(C.byref(got), C.c_void_p)))
    return Q2


def fry_divisors(rss, nf, p, standardize="posterior.sd") -> np.ndarray:
    """plaidhip_fry_divisors on the host: rss nfit x rows, nf per fit -> c_g nfit x rows (NaN: outside the universe)"""
    rss = np.ascontiguousarray(np.atleast_2d(np.asarray(rss, dtype=np.float64)))
    nfit, rows = rss.shape
    nf = np.ascontiguousarray(np.atleast_1d(nf), dtype=np.int64)
    if nf.shape != (nfit,):
        raise ValueError("fry_divisors: nf has one entry per fit")
    cg = np.full((nfit, rows), -7.0)
    check(_lib.load().plaidhip_fry_divisors(rows, int(p), nfit, _np_ptr(rss), _np_ptr(nf), check_fry_standardize(standardize),
                                            _np_ptr(cg)))
    return cg


def fry_residual_row(x, Q, use, E, c) -> np.ndarray:
    """plaidhip_fry_residual_row on the host: the standardised residuals of one gene at the divisor c"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(len(x), -1))
    E = np.ascontiguousarray(E, dtype=np.float64)
    U = None if use is None else np.ascontiguousarray(np.asarray(use) != 0, dtype=np.int8)
    z = np.full(len(x), -7.0)
    check(_lib.load().plaidhip_fry_residual_row(len(x), Q.shape[1], _np_ptr(x), _np_ptr(Q), None if U is None else _np_ptr(U),
                                                _np_ptr(E), float(c), _np_ptr(z)))
    return z


def fry_finish(dres, cnt, sume, ss, sume2=None, lam1=None, lamD=None, trM=None, froM=None, mixed=None):
    """plaidhip_fry_finish on the host: dres per fit, cnt and ss sets x nfit, sume (and the mixed test's sume2, lam1, lamD,
    trM, froM) sets x q x nfit, mixed per fit or None -> out sets x 7 x q x nfit"""
    sume = np.asarray(sume, dtype=np.float64)
    sume = np.asfortranarray(sume[:, :, None] if sume.ndim == 2 else sume)
    m, q, nfit = sume.shape
    f2 = lambda v: np.asfortranarray(np.asarray(v, dtype=np.float64).reshape((m, nfit), order="F"))
    f3 = lambda v: np.asfortranarray(np.asarray(v, dtype=np.float64).reshape((m, q, nfit), order="F"))
    cnt, ss = f2(cnt), f2(ss)
    dres = np.ascontiguousarray(np.atleast_1d(dres), dtype=np.float64)
    extra = [None] * 5 if mixed is None else [f3(v) for v in (sume2, lam1, lamD, trM, froM)]
    mx = None if mixed is None else np.ascontiguousarray(np.atleast_1d(mixed), dtype=np.int8)
    out = np.full((m, 7, q, nfit), -7.0, order="F")
    check(_lib.load().plaidhip_fry_finish(m, nfit, q, _np_ptr(dres), _np_ptr(cnt), _np_ptr(sume), _np_ptr(ss),
                                          *[None if v is None else _np_ptr(v) for v in extra],
                                          None if mx is None else _np_ptr(mx), _np_ptr(out)))
    return out


def beta_upper(x, a, b) -> float:
    """pbeta(x, a, b, lower.tail = FALSE) as plaid.fry's mixed test takes it (a test hook of the library)"""
    f = _lib.load().plaidhip_debug_beta_upper
    f.argtypes, f.restype = [C.c_double] * 3, C.c_double
    return float(f(float(x), float(a), float(b)))


ROAST_COLUMNS = ("NGenes", "PropDown", "PropUp", "Direction", "PValue", "FDR", "PValue.Mixed", "FDR.Mixed")
ROAST_HYPER = LIMMA_HYPER + ("n.genes", "nrot", "mean50.capped")
ROAST_STATISTIC = {"mean": 0, "floormean": 1, "msq": 2, "mean50": 3}
ROAST_ZSCORE = {"hill": 0, "none": 1}
ROAST_MEAN50_MAX = 16384


def check_roast_options(set_statistic, zscore):
    """(set_statistic, zscore) as the C ABI takes them"""
    if set_statistic not in ROAST_STATISTIC:
        raise ValueError(f"roast: set_statistic must be one of {sorted(ROAST_STATISTIC)}")
    if zscore not in ROAST_ZSCORE:
        raise ValueError(f"roast: zscore must be one of {sorted(ROAST_ZSCORE)} (the exact qnorm(pt()) is not offered)")
    return ROAST_STATISTIC[set_statistic], ROAST_ZSCORE[zscore]


def _roast(fn, head, X, design, Gp, Gi, use=None, contrasts=None, set_statistic="mean50", nrot=1999, seed=1, zscore="hill",
           midp=True, rotations=None, out=None, hyper=None):
    """plaidhip_roast / _multi / the hook: (out, hyper) -- sets x 8 x q x nfit (ROAST_COLUMNS) and nfit x 7 (ROAST_HYPER).
    rotations: None (generated from `seed`) or (n + 1) x nrot (x nfit), row 0 = r0"""
    X = _as_f64_fortran(X)
    if X.ndim != 2:
        raise ValueError("roast: the matrix must be genes x samples")
    g, n = X.shape
    D, U, K, q = limma_operands(n, design, use, contrasts)
    p, nfit = D.shape[1], D.shape[2]
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    m = len(Gp) - 1
    stat, zs = check_roast_options(set_statistic, zscore)
    Wr = None
    if rotations is not None:
        Wr = np.asarray(rotations, dtype=np.float64)
        Wr = Wr[:, :, None] if Wr.ndim == 2 else Wr
        if Wr.ndim != 3 or Wr.shape[0] != n + 1 or Wr.shape[2] != nfit:
            raise ValueError("roast: rotations must be (samples + 1) x nrot (x fits)")
        nrot = Wr.shape[1]
        Wr = np.ascontiguousarray(Wr.transpose(2, 0, 1))   # [fit][n + 1][nrot]
    out = np.full((m, 8, q, nfit), np.nan, dtype=np.float64, order="F") if out is None else out
    hyper = np.full((nfit, 7), np.nan, dtype=np.float64) if hyper is None else hyper
    check(fn(*head, _np_ptr(X), g, n, _np_ptr(D), p, nfit, None if U is None else _np_ptr(U), None if K is None else _np_ptr(K),
             q, _np_ptr(Gp), _np_ptr(Gi), m, stat, zs, int(nrot), int(seed), int(bool(midp)), None if Wr is None else _np_ptr(Wr),
             _np_ptr(out), _np_ptr(hyper)))
    return out, hyper


def roast_rotations(design, use=None, fit=0, nrot=1999, seed=1) -> np.ndarray:
    """plaidhip_roast_rotations on the host (no device is touched): W, (n + 1) x nrot, of one design and fit number `fit`
    (from 0): row 0 is r0, row c + 1 the weight of sample c (0.0 where the fit leaves it out)"""
    D0 = np.asarray(design, dtype=np.float64)
    if D0.ndim != 2:
        raise ValueError("roast_rotations: one design, samples x coefficients")
    D, U, _, _ = limma_operands(D0.shape[0], D0, use, None)
    n, p = D.shape[0], D.shape[1]
    W = np.full((n + 1, max(int(nrot), 0)), np.nan)
    check(_lib.load().plaidhip_roast_rotations(_np_ptr(D), n, p, None if U is None else _np_ptr(U), int(fit), int(nrot), int(seed),
                                               _np_ptr(W)))
    return W


def roast_finish(cnt, msize, ndown, nup, nrot, set_statistic="mean50", midp=True):
    """plaidhip_roast_finish on the host: cnt sets x 4 (x q x nfit) integer counts (down, up, upordown, mixed), msize sets
    (x nfit), ndown and nup sets (x q x nfit) -> out sets x 8 x q x nfit"""
    cnt = np.asarray(cnt)
    cnt = cnt[:, :, None, None] if cnt.ndim == 2 else cnt
    m, _, q, nfit = cnt.shape
    cn = np.ascontiguousarray(cnt.transpose(3, 2, 0, 1), dtype=np.int32)   # [fit][contrast][set][4]
    f2 = lambda v: np.asfortranarray(np.asarray(v, dtype=np.float64).reshape((m, nfit), order="F"))
    f3 = lambda v: np.asfortranarray(np.asarray(v, dtype=np.float64).reshape((m, q, nfit), order="F"))
    ms, nd, nu = f2(msize), f3(ndown), f3(nup)
    out = np.full((m, 8, q, nfit), -7.0, order="F")
    check(_lib.load().plaidhip_roast_finish(m, nfit, q, int(nrot), ROAST_STATISTIC[set_statistic], int(bool(midp)), _np_ptr(cn),
                                            _np_ptr(ms), _np_ptr(nd), _np_ptr(nu), _np_ptr(out)))
    return out


ROMER_COLUMNS = ("NGenes", "Up", "Down", "Mixed", "FDR.Up", "FDR.Down", "FDR.Mixed")
ROMER_HYPER = LIMMA_HYPER + ("n.genes", "nrot", "mean50.capped", "nan.t")   # then pi of every contrast
ROMER_STATISTIC = {"mean": 0, "floormean": 1, "mean50": 2}
ROMER_MAX_GENES = 131072


def check_romer_options(set_statistic):
    """set_statistic as the C ABI takes it"""
    if set_statistic not in ROMER_STATISTIC:
        raise ValueError(f"romer: set_statistic must be one of {sorted(ROMER_STATISTIC)}")
    return ROMER_STATISTIC[set_statistic]


def _romer(fn, head, X, design, Gp, Gi, use=None, contrasts=None, set_statistic="mean", nrot=9999, seed=1, shrink_resid=True,
           shrink=None, rotations=None, out=None, hyper=None):
    """plaidhip_romer / _multi / the hook: (out, hyper) -- sets x 7 x q x nfit (ROMER_COLUMNS) and nfit x (8 + q) (ROMER_HYPER,
    then pi of every contrast).  rotations: None (generated from `seed`) or (n + 1) x nrot (x nfit), row 0 = r0; shrink: None
    or the factors, genes x q (x nfit)"""
    X = _as_f64_fortran(X)
    if X.ndim != 2:
        raise ValueError("romer: the matrix must be genes x samples")
    g, n = X.shape
    D, U, K, q = limma_operands(n, design, use, contrasts)
    p, nfit = D.shape[1], D.shape[2]
    Gp, Gi = _as_i32(Gp), _as_i32(Gi)
    m = len(Gp) - 1
    stat = check_romer_options(set_statistic)
    Wr = None
    if rotations is not None:
        Wr = np.asarray(rotations, dtype=np.float64)
        Wr = Wr[:, :, None] if Wr.ndim == 2 else Wr
        if Wr.ndim != 3 or Wr.shape[0] != n + 1 or Wr.shape[2] != nfit:
            raise ValueError("romer: rotations must be (samples + 1) x nrot (x fits)")
        nrot = Wr.shape[1]
        Wr = np.ascontiguousarray(Wr.transpose(2, 0, 1))   # [fit][n + 1][nrot]
    Sh = None
    if shrink is not None:
        Sh = np.asarray(shrink, dtype=np.float64)
        Sh = Sh[:, None] if Sh.ndim == 1 else Sh
        Sh = Sh[:, :, None] if Sh.ndim == 2 else Sh
        if Sh.shape != (g, q, nfit):
            raise ValueError("romer: shrink must be genes x contrasts (x fits)")
        Sh = np.asfortranarray(Sh)
    out = np.full((m, 7, q, nfit), np.nan, dtype=np.float64, order="F") if out is None else out
    hyper = np.full((nfit, 8 + q), np.nan, dtype=np.float64) if hyper is None else hyper
    check(fn(*head, _np_ptr(X), g, n, _np_ptr(D), p, nfit, None if U is None else _np_ptr(U), None if K is None else _np_ptr(K),
             q, _np_ptr(Gp), _np_ptr(Gi), m, stat, int(nrot), int(seed), int(bool(shrink_resid)), None if Sh is None else _np_ptr(Sh),
             None if Wr is None else _np_ptr(Wr), _np_ptr(out), _np_ptr(hyper)))
    return out, hyper


def romer_shrink(t, u, s02, nu):
    """plaidhip_romer_shrink on the host (no device is touched): (c, pi) -- the factors of the genes with moderated t `t` of
    one (fit, contrast) with stdev.unscaled u, prior variance s02 and nu = df.prior + df.residual (may be inf)"""
    t = np.ascontiguousarray(t, dtype=np.float64)
    c = np.full(t.shape, np.nan)
    prop = np.full(1, np.nan)
    check(_lib.load().plaidhip_romer_shrink(len(t), _np_ptr(t), float(u), float(s02), float(nu), _np_ptr(c), _np_ptr(prop)))
    return c, float(prop[0])


def romer_finish(cnt, msize, nrot, set_statistic="mean"):
    """plaidhip_romer_finish on the host: cnt sets x 3 (x q x nfit) integer counts (Up, Down, Mixed), msize sets (x nfit) ->
    out sets x 7 x q x nfit"""
    cnt = np.asarray(cnt)
    cnt = cnt[:, :, None, None] if cnt.ndim == 2 else cnt
    m, _, q, nfit = cnt.shape
    cn = np.ascontiguousarray(cnt.transpose(3, 2, 0, 1), dtype=np.int32)   # [fit][contrast][set][3]
    ms = np.asfortranarray(np.asarray(msize, dtype=np.float64).reshape((m, nfit), order="F"))
    out = np.full((m, 7, q, nfit), -7.0, order="F")
    check(_lib.load().plaidhip_romer_finish(m, nfit, q, int(nrot), ROMER_STATISTIC[set_statistic], _np_ptr(cn), _np_ptr(ms),
                                            _np_ptr(out)))
    return out


class Context:
    """plaidhip_ctx: one device + one stream.  `stream` is a raw hipStream_t value (e.g.
    `torch.cuda.current_stream().cuda_stream`; 0 is the device's null stream, which is what torch's default
    stream is) or None for a private non-blocking stream."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.plaidhip_init(int(device), None, C.byref(h)))
        self.handle = h
        self.device = int(device)
        self.stream = None
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream: int):
        """enqueue on this hipStream_t from now on (0: the null stream)"""
        check(self.lib.plaidhip_set_stream(self.handle, C.c_void_p(int(stream)) if stream else None))
        self.stream = int(stream)

    def set_option(self, name: str, value):
        """kernel-selection knobs (plaidhip_set_option): see _lib.OPTIONS"""
        code, values = _lib.OPTIONS[name]
        check(self.lib.plaidhip_set_option(self.handle, code, values[value] if isinstance(value, str) else int(value)))

    def limit(self, name: str) -> int:
        """size limits a host routes by (plaidhip_limit): "sparse_rank_column", "lds_genes" """
        v = C.c_int64(0)
        check(self.lib.plaidhip_limit({"sparse_rank_column": 1, "lds_genes": 2}[name], C.byref(v)))
        return int(v.value)

    def close(self):
        if self.handle:
            self.lib.plaidhip_finalize(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self.lib.plaidhip_synchronize(self.handle))

    def set_precision(self, mode: str):
        """"f64" (default): fp64 throughout.  "mixed": the dense crossprod stages the sample columns as fp32
        (inputs rounded to 2^-24 relative, four-term fp32 partial sums accumulated in fp64: 3 * 2^-24 of sum |x| plus the
        fp64 bound, include/plaidhip.h) -- about 2x the SpMM rate, scores within ~1e-7."""
        check(self.lib.plaidhip_set_precision(self.handle, {"f64": 0, "mixed": 1}[mode]))

    def geneset(self, g: int, Gp, Gi) -> Geneset:
        return Geneset(self, g, Gp, Gi)

    # ---- device-level (raw device pointers) ------------------------------------------
    def dev_spmm_dense(self, gs: Geneset, X: int, ldx: int, n: int, S: int, lds: int, stat="mean",
                       alpha=1.0, beta=0.0, flags: int | None = None, alpha_div: int | None = None):
        check(self.lib.plaidhip_dev_spmm_dense_f64(self.handle, gs.handle, X, ldx, n, STAT[stat], alpha,
                                                   alpha_div, beta, S, lds, flags))

    def dev_spmm_dense_fused(self, gs: Geneset, X: int, ldx: int, n: int, S: int, lds: int, stat="mean",
                             alpha=1.0, beta=0.0, flags: int | None = None, alpha_div: int | None = None) -> int:
        """dev_spmm_dense that also classifies the scores for normalize_medians while it writes them (the fp64 pair
        kernel, more than 6,144 sets per column, >= 1e9 scores or fused_medians = on); dev_col_medians_resume then
        finishes the medians without a second pass over S.  Returns the launch's token (0: the plain route ran)"""
        check(self.lib.plaidhip_dev_spmm_dense_fused_f64(self.handle, gs.handle, X, ldx, n, STAT[stat], alpha,
                                                         alpha_div, beta, S, lds, flags))
        return self.dev_fused_medians_token()

    def dev_spmm_ranks(self, gs: Geneset, R: int, ldr: int, n: int, S: int, lds: int, stat="mean",
                       alpha=1.0, beta=0.0, flags: int | None = None, alpha_div: int | None = None):
        """the crossprod of a RANK matrix (what dev_colranks_dense wrote with power 1, unsigned): u16 staging, integer
        sums -- bit-identical to dev_spmm_dense on the same input"""
        check(self.lib.plaidhip_dev_spmm_ranks_f64(self.handle, gs.handle, R, ldr, n, STAT[stat], alpha,
                                                   alpha_div, beta, S, lds, flags))

    def debug_spec_fell_back(self) -> bool:
        """test hook (plaidhip_debug_spec_fell_back, read-only; waits for the stream): True when the last speculative
        u16 launch of this context met a value that is not a rank and the fp64 kernel behind it recomputed the scores"""
        out = C.c_int(0)
        check(self.lib.plaidhip_debug_spec_fell_back(self.handle, C.byref(out)))
        return bool(out.value)

    def dev_spmm_csc(self, gs: Geneset, Xp: int, Xi: int, Xx: int, n: int, S: int, lds: int,
                     stat="mean", alpha=1.0, beta=0.0, flags: int | None = None,
                     alpha_div: int | None = None, nnz: int = -1):
        """nnz: stored values of X when the caller knows it (one kernel is launched), -1: decided on the device"""
        check(self.lib.plaidhip_dev_spmm_csc_f64(self.handle, gs.handle, Xp, Xi, Xx, n, int(nnz), STAT[stat], alpha,
                                                 alpha_div, beta, S, lds, flags))

    def dev_spmm_csc_ranks(self, gs: Geneset, Xp: int, Xi: int, Rx: int, n: int, S: int, lds: int, rmax: int,
                           stat="mean", alpha=1.0, beta=0.0, flags: int | None = None, nnz: int = -1):
        """the sparse crossprod of rank weights (0 <= Rx <= *rmax, what dev_colranks_csc wrote; alpha is divided by
        *rmax): order-independent fixed-point sums in the scatter kernel"""
        check(self.lib.plaidhip_dev_spmm_csc_ranks_f64(self.handle, gs.handle, Xp, Xi, Rx, n, int(nnz), STAT[stat], alpha,
                                                       rmax, beta, S, lds, flags))

    def dev_spmm_csc_fused(self, gs: Geneset, Xp: int, Xi: int, Xx: int, n: int, S: int, lds: int, stat="mean", alpha=1.0,
                           beta=0.0, flags: int | None = None, alpha_div: int | None = None, rmax: int | None = None,
                           nnz: int = -1):
        """dev_spmm_csc (rmax None) / dev_spmm_csc_ranks (rmax set) that also classifies the scores for
        normalize_medians while it writes them; dev_col_medians_resume then finishes the medians without a second pass
        over S (plaidhip_dev_spmm_csc_fused_f64)"""
        check(self.lib.plaidhip_dev_spmm_csc_fused_f64(self.handle, gs.handle, Xp, Xi, Xx, n, int(nnz), STAT[stat], alpha,
                                                       alpha_div, beta, S, lds, flags, rmax))
        return self.dev_fused_medians_token()

    def dev_col_medians_resume(self, S: int, lds: int, m: int, n: int, ignore_zero, med: int, flags: int | None = None,
                               token: int | None = None):
        """dev_col_medians for the S the last dev_spmm_csc_fused on this context wrote.  `token` (what dev_spmm_csc_fused
        returned): the candidates are used only while they are the pending ones of that very launch; None = the caller
        resumes directly after the crossprod (S recognised by pointer and shape)"""
        iz = -1 if ignore_zero is None else int(bool(ignore_zero))
        if token is None:
            check(self.lib.plaidhip_dev_col_medians_resume(self.handle, S, lds, m, n, iz, flags, med))
        else:
            check(self.lib.plaidhip_dev_col_medians_resume_token(self.handle, int(token), S, lds, m, n, iz, flags, med))

    def dev_fused_medians_discard(self):
        check(self.lib.plaidhip_dev_fused_medians_discard(self.handle))

    def dev_fused_medians_token(self) -> int:
        """token of the pending fused launch (0: none -- the plain route ran, or it was consumed / superseded)"""
        return self.dev_fused_medians_info()[3]

    def dev_fused_medians_info(self):
        """(columns of the last fused crossprod or 0, device pointer of status[n], device pointer of the calibration,
        token of the pending launch or 0)"""
        buf = (C.c_int64 * 4)()
        check(self.lib.plaidhip_dev_fused_medians_info(self.handle, buf))
        return int(buf[0]), int(buf[1]), int(buf[2]), int(buf[3])

    def dev_crossprod_weighted(self, Wp: int, Wi: int, Wx: int, g: int, m: int, Y: int, ldy: int, n: int, S: int,
                               lds: int):
        """t(x) %*% y for a sparse x with arbitrary stored values (device dgCMatrix slots), y dense"""
        check(self.lib.plaidhip_dev_crossprod_weighted_f64(self.handle, Wp, Wi, Wx, int(g), int(m), Y, int(ldy), int(n),
                                                           S, int(lds)))

    def dev_crossprod_weighted_csc(self, Wp: int, Wi: int, Wx: int, g: int, m: int, Yp: int, Yi: int, Yx: int,
                                   n: int, S: int, lds: int):
        check(self.lib.plaidhip_dev_crossprod_weighted_csc_f64(self.handle, Wp, Wi, Wx, int(g), int(m), Yp, Yi, Yx,
                                                               int(n), S, int(lds)))

    def dev_colranks_dense(self, X: int, ldx: int, g: int, n: int, R: int, ldr: int, ties="average",
                           signed=False, power=1.0, colmax: int | None = None):
        check(self.lib.plaidhip_dev_colranks_dense_f64(self.handle, X, ldx, g, n, TIES[ties], int(signed),
                                                       power, R, ldr, colmax))

    def dev_colranks_csc(self, Xp: int, Xx: int, n: int, max_col_nnz: int, Rx: int, ties="average", signed=False,
                         power=1.0, colmax: int | None = None):
        """max_col_nnz: upper bound on the stored values of a column (sizes the launch; nrow(X) is always valid)"""
        check(self.lib.plaidhip_dev_colranks_csc_f64(self.handle, Xp, Xx, n, int(max_col_nnz), TIES[ties], int(signed),
                                                     power, Rx, colmax))

    def dev_colranks_csc_dense(self, Xp: int, Xi: int, Xx: int, g: int, n: int, R: int, ldr: int, ties="average",
                               signed=False, power=1.0, colmax: int | None = None):
        """dense ranks of CSC columns (zeros ranked) by densify-and-rank: columns with any number of stored values"""
        check(self.lib.plaidhip_dev_colranks_csc_dense_f64(self.handle, Xp, Xi, Xx, int(g), int(n), TIES[ties], int(signed),
                                                           power, R, int(ldr), colmax))

    def debug_rank_fallbacks(self):
        """test hook (plaidhip_debug_rank_fallbacks, read-only; waits for the stream): the number of columns the last rank
        launch of this context handed to the sorting network -- (by the bucket ranker, by the value-partitioned ranker);
        -1 where that launcher did not run with a hand-over list"""
        out = (C.c_int32 * 2)()
        check(self.lib.plaidhip_debug_rank_fallbacks(self.handle, out))
        return int(out[0]), int(out[1])

    def dev_colranks_csc_dense_nz(self, Xp: int, Xi: int, Xx: int, g: int, n: int, max_col_nnz: int, Rx_scratch: int, R: int,
                                  ldr: int, ties="average", signed=False, power=1.0, colmax: int | None = None):
        """dense ranks of CSC columns (zeros ranked) from the ranks of the stored values: any nrow(X); Rx_scratch: Xp[n]
        doubles; every column at most 20,352 stored values"""
        check(self.lib.plaidhip_dev_colranks_csc_dense_nz_f64(self.handle, Xp, Xi, Xx, int(g), int(n), int(max_col_nnz),
                                                              TIES[ties], int(signed), power, Rx_scratch, R, int(ldr), colmax))

    def dev_ssgsea_exact_operands(self, X: int, ldx: int, g: int, n: int, alpha: float, Q: int, ldq: int, scratch: int,
                                  colnan: int, W: int | None = None, P: int | None = None):
        """replaid.ssgsea.exact's operands of dense columns: Q = last ranks, W = average ranks ^ alpha, P = W * Q (W, P
        needed when alpha != 0), colnan[c] = 1 for a column with a NaN; scratch: 2 ldq n doubles"""
        check(self.lib.plaidhip_dev_ssgsea_exact_operands_f64(self.handle, X, int(ldx), int(g), int(n), float(alpha), Q, W, P,
                                                              int(ldq), scratch, colnan))

    def dev_ssgsea_exact_operands_csc(self, Xp: int, Xi: int, Xx: int, g: int, n: int, max_col_nnz: int, nnz: int,
                                      alpha: float, Q: int, ldq: int, scratch: int, colnan: int, W: int | None = None,
                                      P: int | None = None):
        """the same for the device slots of a dgCMatrix (dense results, zeros ranked); scratch: 3 nnz doubles"""
        check(self.lib.plaidhip_dev_ssgsea_exact_operands_csc_f64(self.handle, Xp, Xi, Xx, int(g), int(n), int(max_col_nnz),
                                                                  int(nnz), float(alpha), Q, W, P, int(ldq), scratch, colnan))

    def dev_gsea_ks(self, Q: int, ldq: int, colnan: int, g: int, n: int, Gp: int, Gi: int, m: int, alpha: float,
                    scale: bool, S: int, lds: int, W: int | None = None):
        """the walk of replaid.ssgsea.exact(single = FALSE) on device operands (dev_ssgsea_exact_operands' Q, W, colnan)
        and a device copy of the aligned pattern: S (m x n) = the running sum's value of largest magnitude; W is needed
        when alpha != 0"""
        check(self.lib.plaidhip_dev_gsea_ks_f64(self.handle, Q, W, int(ldq), colnan, int(g), int(n), Gp, Gi, int(m),
                                                float(alpha), int(bool(scale)), S, int(lds)))

    def dev_gsva_ks(self, Q: int, ldq: int, colnan: int, g: int, n: int, Gp: int, Gi: int, m: int, tau: float,
                    max_diff: bool, S: int, lds: int):
        """the walk of replaid.gsva.exact on the device's last ranks of the row-transformed columns
        (dev_ssgsea_exact_operands with alpha = 0: Q, colnan) and a device copy of the aligned pattern: S (m x n)"""
        check(self.lib.plaidhip_dev_gsva_ks_f64(self.handle, Q, int(ldq), colnan, int(g), int(n), Gp, Gi, int(m), float(tau),
                                                int(bool(max_diff)), S, int(lds)))

    def dev_sing_mad(self, R: int, Q: int, ldq: int, colnan: int, g: int, n: int, Gp: int, Gi: int, m: int, S: int, lds: int):
        """the dispersion of replaid.sing.exact on the device's min ranks R (dev_colranks_dense, ties "min"), last ranks Q
        and NaN flags (dev_ssgsea_exact_operands with alpha = 0) and a device copy of the aligned pattern: S (m x n)"""
        check(self.lib.plaidhip_dev_sing_mad_f64(self.handle, R, Q, int(ldq), colnan, int(g), int(n), Gp, Gi, int(m), S,
                                                 int(lds)))

    def dev_minflags(self, S: int, count: int, flags: int):
        check(self.lib.plaidhip_dev_minflags(self.handle, S, count, flags))

    def dev_col_medians(self, S: int, lds: int, m: int, n: int, ignore_zero, med: int,
                        flags: int | None = None):
        """ignore_zero: True / False, or None to resolve min(x)==0 on the device from `flags`."""
        iz = -1 if ignore_zero is None else int(bool(ignore_zero))
        check(self.lib.plaidhip_dev_col_medians(self.handle, S, lds, m, n, iz, flags, med))

    def dev_sum(self, v: int, count: int, out: int):
        check(self.lib.plaidhip_dev_sum(self.handle, v, count, out))

    def dev_max(self, v: int, count: int, out: int):
        check(self.lib.plaidhip_dev_max(self.handle, v, count, out))

    def dev_shift_columns(self, S: int, lds: int, m: int, n: int, med: int, add: float = 0.0,
                          red: int | None = None):
        """x - med[col] + add; with `red` (device {sum, count}) add = sum/count on the device."""
        check(self.lib.plaidhip_dev_shift_columns(self.handle, S, lds, m, n, med, float(add), red))

    def dev_shift_columns_cast_f32(self, S: int, lds: int, m: int, n: int, med: int, out: int, ldo: int, add: float = 0.0,
                                   red: int | None = None):
        """out (float32) = x - med[col] + add, S untouched: the shift fused with the cast a sharded gather makes"""
        check(self.lib.plaidhip_dev_shift_columns_cast_f32(self.handle, S, lds, m, n, med, float(add), red, out, ldo))

    def dev_row_group_sums(self, A: int, ld: int, rows: int, n: int, y: int, sums: int):
        """per-row sums over the columns with y == 0 / y == 1 -> sums[2][rows] (plaid.test, R/plaid.R:407-408, 431)"""
        check(self.lib.plaidhip_dev_row_group_sums(self.handle, A, ld, rows, n, y, sums))

    def dev_row_contrast_sums(self, A: int, ld: int, rows: int, n: int, Y: int, C: int, sums: int):
        """dev_row_group_sums for the C label columns of Y (n x C int32, column-major) at once; sums: [C][2][rows]"""
        check(self.lib.plaidhip_dev_row_contrast_sums(self.handle, A, ld, rows, n, Y, C, sums))

    def dev_row_contrast_ssd(self, A: int, ld: int, rows: int, n: int, Y: int, C: int, mean: int, ssd: int):
        """dev_row_group_ssd for C label columns at once; mean, ssd: [C][2][rows]"""
        check(self.lib.plaidhip_dev_row_contrast_ssd(self.handle, A, ld, rows, n, Y, C, mean, ssd))

    def dev_row_group_ssd(self, A: int, ld: int, rows: int, n: int, y: int, mean: int, ssd: int):
        """per-row sums of squared deviations from the given group means -> ssd[2][rows] (R/plaid.R:429)"""
        check(self.lib.plaidhip_dev_row_group_ssd(self.handle, A, ld, rows, n, y, mean, ssd))

    # ---- host-level (numpy in, numpy out; the library stages through HBM) -------------
    _result = staticmethod(_result)

    def _host(self, name, X, Gp, Gi, *tail, **kw):
        return _score(getattr(self.lib, "plaidhip_" + name), (self.handle,), X, Gp, Gi, *tail, **kw)

    def plaid_dense(self, X, Gp, Gi, stat="mean", normalize=True, out=None) -> np.ndarray:
        return self._host("plaid_dense", _as_f64_fortran(X), Gp, Gi, STAT[stat], int(bool(normalize)), dense=True, out=out)

    def plaid_csc(self, Xp, Xi, Xx, g: int, Gp, Gi, stat="mean", normalize=True, out=None) -> np.ndarray:
        return self._host("plaid_csc", _slots(Xp, Xi, Xx, g), Gp, Gi, STAT[stat], int(bool(normalize)), out=out)

    def crossprod_weighted(self, Wp, Wi, Wx, g: int, Y=None, Yp=None, Yi=None, Yx=None) -> np.ndarray:
        """chunked_crossprod's t(x) %*% y for a sparse x with arbitrary stored values (R/plaid.R:100-123); y dense
        (`Y`, g x n) or its dgCMatrix slots"""
        Wp, Wi = _as_i32(Wp), _as_i32(Wi)
        Wx = np.ascontiguousarray(Wx, dtype=np.float64)
        m = len(Wp) - 1
        if Y is not None:
            Y = _as_f64_fortran(Y)
            n = Y.shape[1]
            S = np.empty((m, n), dtype=np.float64, order="F")
            check(self.lib.plaidhip_crossprod_weighted_dense(self.handle, _np_ptr(Wp), _np_ptr(Wi), _np_ptr(Wx), int(g), m,
                                                             _np_ptr(Y), n, _np_ptr(S)))
            return S
        Yp, Yi = _as_i32(Yp), _as_i32(Yi)
        Yx = np.ascontiguousarray(Yx, dtype=np.float64)
        n = len(Yp) - 1
        S = np.empty((m, n), dtype=np.float64, order="F")
        check(self.lib.plaidhip_crossprod_weighted_csc(self.handle, _np_ptr(Wp), _np_ptr(Wi), _np_ptr(Wx), int(g), m,
                                                       _np_ptr(Yp), _np_ptr(Yi), _np_ptr(Yx), n, _np_ptr(S)))
        return S

    def normalize_medians(self, S, ignore_zero=None):
        S = np.array(S, dtype=np.float64, order="F", copy=True)
        m, n = S.shape
        med = np.empty(n, dtype=np.float64)
        iz = -1 if ignore_zero is None else int(bool(ignore_zero))
        check(self.lib.plaidhip_normalize_medians(self.handle, _np_ptr(S), m, n, iz, _np_ptr(med)))
        return S, med

    def colranks_dense(self, X, ties="average", signed=False) -> np.ndarray:
        X = _as_f64_fortran(X)
        g, n = X.shape
        R = np.empty((g, n), dtype=np.float64, order="F")
        check(self.lib.plaidhip_colranks_dense(self.handle, _np_ptr(X), g, n, TIES[ties], int(bool(signed)),
                                               _np_ptr(R)))
        return R

    def colranks_csc(self, Xp, Xx, ties="average", signed=False) -> np.ndarray:
        Xp = _as_i32(Xp)
        Xx = np.ascontiguousarray(Xx, dtype=np.float64)
        R = np.empty(len(Xx), dtype=np.float64)
        check(self.lib.plaidhip_colranks_csc(self.handle, _np_ptr(Xp), _np_ptr(Xx), len(Xp) - 1, TIES[ties],
                                             int(bool(signed)), _np_ptr(R)))
        return R

    def colranks_csc_dense(self, Xp, Xi, Xx, g: int, ties="average", signed=False) -> np.ndarray:
        """colranks(sparse X, keep.zero=FALSE): zeros ranked, dense g x n result (R/plaid.R:602-609)"""
        Xp, Xi = _as_i32(Xp), _as_i32(Xi)
        Xx = np.ascontiguousarray(Xx, dtype=np.float64)
        n = len(Xp) - 1
        R = np.empty((int(g), n), dtype=np.float64, order="F")
        check(self.lib.plaidhip_colranks_csc_dense(self.handle, _np_ptr(Xp), _np_ptr(Xi), _np_ptr(Xx), int(g), n,
                                                   TIES[ties], int(bool(signed)), _np_ptr(R)))
        return R

    def sing_dense(self, X, Gp, Gi) -> np.ndarray:
        return self._host("sing_dense", _as_f64_fortran(X), Gp, Gi, dense=True)

    def sing_csc(self, Xp, Xi, Xx, g: int, Gp, Gi) -> np.ndarray:
        """replaid.sing for a dgCMatrix X (zeros are ranked, R/plaid.R:215-217 with colranks' sparse branch :602-609)"""
        return self._host("sing_csc", _slots(Xp, Xi, Xx, g), Gp, Gi)

    def ssgsea_dense(self, X, Gp, Gi, alpha=0.0) -> np.ndarray:
        return self._host("ssgsea_dense", _as_f64_fortran(X), Gp, Gi, float(alpha), dense=True)

    def ssgsea_csc(self, Xp, Xi, Xx, g: int, Gp, Gi, alpha=0.0) -> np.ndarray:
        return self._host("ssgsea_csc", _slots(Xp, Xi, Xx, g), Gp, Gi, float(alpha))

    def ucell(self, X, Gp, Gi, k_full, rmax=1500.0):
        kf = np.ascontiguousarray(k_full, dtype=np.float64)
        return self._host("ucell", X, Gp, Gi, _np_ptr(kf), float(rmax))

    def aucell(self, X, Gp, Gi, auc_max_rank):
        return self._host("aucell", X, Gp, Gi, float(auc_max_rank))

    def scse(self, X, Gp, Gi, remove_log2=None, score_mean=False):
        S, self.last_scse_removed_log2 = _scse(self.lib.plaidhip_scse, (self.handle,), X, Gp, Gi, remove_log2, score_mean)
        return S

    def ssgsea_exact(self, X, Gp, Gi, alpha=0.25, scale=True, norm=False, single=True):
        """plaidhip_ssgsea_exact: the original ssGSEA statistic (gao.ssgsea, single = TRUE) for any alpha; X dense or scipy
        CSC (scored as its dense form), G aligned to X's rows.  single = False (plaidhip_ssgsea_exact_ks): the running sum's
        value of largest magnitude, the classic GSEA enrichment score, instead of its sum"""
        return self._host("ssgsea_exact" if single else "ssgsea_exact_ks", X, Gp, Gi, float(alpha), int(bool(scale)),
                           int(bool(norm)))

    def gsva_exact(self, X, Gp, Gi, tau=1.0, rowtf="z", max_diff=True):
        """plaidhip_gsva_exact: GSVA's random-walk statistic for any tau >= 0; rowtf "z" / "ecdf" (replaid.gsva's row
        transforms), "none" or "gauss" (GSVA's Gaussian kernel CDF estimate: gsva_kcdf; at least 2 samples); X dense or scipy
        CSC with sorted, distinct row indices (scored as its dense form), G aligned to X's rows"""
        return self._host("gsva_exact", X, Gp, Gi, *check_gsva_exact_args(tau, rowtf), int(bool(max_diff)))

    def gsva_kcdf(self, X):
        """plaidhip_gsva_kcdf: V (genes x samples), GSVA's Gaussian kernel CDF estimate of every value among its gene's
        samples (bandwidth sd / 4, the sums of include/plaidhip.h in sample order), the row transform "gauss" of gsva_exact;
        X dense or scipy CSC (expanded on the device, the bits of its dense form); at least 2 samples"""
        xp, xi, xv, g, n, keep = _x_args(X)
        if n < 2:
            raise ValueError(f"gsva_kcdf: the kernel CDF estimate needs at least 2 samples (got {n})")
        V = np.empty((g, n), dtype=np.float64, order="F")
        check(self.lib.plaidhip_gsva_kcdf(self.handle, xp, xi, xv, g, n, _np_ptr(V)))
        return V

    @staticmethod
    def gsva_kcdf_table() -> np.ndarray:
        return gsva_kcdf_table()

    def sing_exact(self, X, Gp, Gi, Dp=None, Di=None, center=True, dispersion=True):
        """plaidhip_sing_exact: singscore's normalised score and dispersion (the MAD of the set's ranks) per set and sample;
        X dense or scipy CSC with sorted, distinct row indices (scored as its dense form), the up sets G and the down sets D
        (optional, as many columns) aligned to X's rows.  A dict of m x n matrices: UpScore [, UpDispersion], and with down
        sets TotalScore, DownScore [, TotalDispersion, DownDispersion].  dispersion = False launches no per-pair kernel."""
        return _sing_exact_call(self.lib.plaidhip_sing_exact, (self.handle,), X, Gp, Gi, Dp, Di, center, dispersion)

    def ucell_exact(self, X, Gp, Gi, Dp=None, Di=None, max_rank=1500, w_neg=1.0, k_full=None, k_full_down=None):
        """plaidhip_ucell_exact: UCell's statistic on truncated ranks; X dense or scipy CSC with sorted, distinct row indices
        (never expanded), the up sets G and the down sets D (optional, as many columns) aligned to X's rows.  k_full (and
        k_full_down): the set sizes before the alignment (UCell's missing_genes = "impute"); None: the aligned sizes.  A
        dict of m x n matrices: UpScore, and with down sets TotalScore (up - w_neg * down, clamped at 0) and DownScore."""
        return _ucell_exact_call(self.lib.plaidhip_ucell_exact, (self.handle,), X, Gp, Gi, Dp, Di, max_rank, w_neg, k_full,
                                 k_full_down)

    def aucell_exact(self, X, Gp, Gi, auc_max_rank):
        """plaidhip_aucell_exact: AUCell's AUC on truncated ranks, ties broken by row order; X dense or scipy CSC with sorted,
        distinct row indices (never expanded), G aligned to X's rows"""
        return self._host("aucell_exact", X, Gp, Gi, float(auc_max_rank))

    def gsea(self, stat, weight, Gp, Gi, perm=None, nperm=1000, seed=1, null=False, score_type="std", leading_edge=False):
        """plaidhip_gsea: preranked GSEA of the columns of stat (genes x lists) with their weights; perm: genes x nperm
        int32 placements, or None for the placements generated from `seed`.  Returns sets x 12 x lists (GSEA_COLUMNS); with
        null = True also the sets x nperm x lists null scores.  score_type "pos" / "neg" (plaidhip_gsea_scored) scores one
        side of the walk; leading_edge = True appends le_len (sets x lists int32) and le_idx (Gp[-1] x lists int32: the edge
        of set j in list l is le_idx[Gp[j]:Gp[j] + le_len[j, l], l], rows of stat, -1 behind it)."""
        if gsea_score_type(score_type) == 0 and not leading_edge:
            return _gsea(self.lib.plaidhip_gsea, (self.handle,), stat, weight, Gp, Gi, perm, nperm, seed, null)
        return _gsea(self.lib.plaidhip_gsea_scored, (self.handle,), stat, weight, Gp, Gi, perm, nperm, seed, null, score_type,
                     leading_edge)

    def gsea_multilevel(self, stat, weight, Gp, Gi, perm=None, nperm=1000, seed=1, null=False, score_type="std",
                        leading_edge=False, sample_size=101, sweeps=4, eps=1e-50, ml_min=10):
        """plaidhip_gsea_multilevel: Context.gsea with multilevel p-values where fewer than ml_min permutations were as
        extreme: (out, ml[, null][, le_len, le_idx]) -- out sets x 12 x lists with the reported pval and padj, ml sets x 6 x
        lists (GSEA_ML_COLUMNS: pvalML, log2err, the read-off stage, the status as an index of GSEA_ML_STATUS, qhat, denom)"""
        return _gsea_multilevel(self.lib.plaidhip_gsea_multilevel, (self.handle,), stat, weight, Gp, Gi, perm, nperm, seed, null,
                                score_type, leading_edge, sample_size, sweeps, eps, ml_min)

    def gsea_ruler(self, stat, weight, k, l=0, side=0, score_type="std", gamma=2.0, seed=1, sample_size=101, sweeps=4, eps=1e-50):
        """plaidhip_gsea_ruler: one ruler of one list (stat, weight: genes), set size k, list number l and side (0 positive,
        1 negative), run to the target gamma: {"stages", "status", "m", "s", "h"} -- the levels, the counts above them and the
        stages x sample_size scores of the stages it ran"""
        sample_size, sweeps, eps = check_gsea_ml_args("gsea_ruler", sample_size, sweeps, eps)
        stat, weight = np.ascontiguousarray(stat, dtype=np.float64).ravel(), np.ascontiguousarray(weight, dtype=np.float64).ravel()
        if stat.shape != weight.shape:
            raise ValueError("gsea_ruler: stat and weight must be one list of one length")
        S = GSEA_ML_MAX_STAGES
        nst, end = C.c_int32(0), C.c_int32(0)
        m_out, s_out = np.zeros(S, dtype=np.float64), np.zeros(S, dtype=np.int32)
        h_out = np.zeros((S, sample_size), dtype=np.float64)
        check(self.lib.plaidhip_gsea_ruler(self.handle, _np_ptr(stat), _np_ptr(weight), len(stat), int(k), int(l), int(side),
                                           gsea_score_type(score_type), float(gamma), int(seed) & (2**64 - 1), sample_size, sweeps,
                                           eps, C.byref(nst), C.byref(end), _np_ptr(m_out), _np_ptr(s_out), _np_ptr(h_out)))
        ns = nst.value
        return {"stages": ns, "status": end.value, "m": m_out[:ns].copy(), "s": s_out[:ns].copy(), "h": h_out[:ns].copy()}

    def limma(self, A, design, use=None, contrasts=None, na="propagate", max_na=0.2, weights=None):
        """plaidhip_limma: moderated t-tests of the rows of A (rows x samples) for the designs (samples x p, or x p x nfit),
        the samples `use` leaves out (samples x nfit, None: none) and the contrasts (p x q, None: every coefficient):
        (out rows x 6 x q x nfit in LIMMA_COLUMNS, hyper nfit x 4 in LIMMA_HYPER).  na = "fit" (plaidhip_limma_na): rows with at
        most the share max_na of NaN are refitted on the samples they have, and the result is (out, hyper nfit x 5 in
        LIMMA_HYPER_NA, dfres rows x nfit: the df.residual of every fitted row, NaN for the others); at most
        LIMMA_NA_MAX_COEF coefficients.  weights (plaidhip_limma_w): a rows x samples matrix of observation weights, a vector
        of array weights, or a pair of both; an observation with a NaN value or a weight that is not positive and finite is
        missing, the result is that of na = "fit", and na = "propagate" stands for max_na = 0 (no row with a NaN is fitted)"""
        return _limma_any(self.lib.plaidhip_limma, self.lib.plaidhip_limma_na, (self.handle,), A, design, use, contrasts, na,
                          max_na, weights, self.lib.plaidhip_limma_w)

    def voom(self, counts, design, lib_size=None, span=0.5):
        """plaidhip_voom: limma's voom (normalize.method = "none") of a counts matrix (rows x samples) for one design: dict of E
        (log2-CPM), weights, lib_size, offset, knots_x, knots_y.  Context.limma(E, design, weights=weights) is the fit"""
        return _voom(self.lib.plaidhip_voom, (self.handle,), counts, design, lib_size, span)

    def dev_voom_weights(self, Q: int, offset: int, n: int, p: int, Eff: int, rows: int, kx: int, ky: int, nk: int, W: int, ldw: int):
        """plaidhip_dev_voom_weights on device pointers: W rows x n (leading dimension ldw) from the effects Eff [p + 1][rows]"""
        check(self.lib.plaidhip_dev_voom_weights(self.handle, Q, offset, n, p, Eff, rows, kx, ky, nk, W, ldw))

    def dev_limma_w_sums(self, A: int, Wt, aw, ld: int, rows: int, n: int, Q: int, use, invn: int, p: int, nfit: int, seed, S: int,
                         seed_cnt=None, cnt=None):
        """plaidhip_dev_limma_w_sums on device pointers: S [nfit (p (p + 1) / 2 + p + 1)][rows], cnt [2 nfit + 1][rows] or None;
        Wt, aw, use and the seeds may be None"""
        check(self.lib.plaidhip_dev_limma_w_sums(self.handle, A, Wt, aw, ld, rows, n, Q, use, invn, p, nfit, seed, S, seed_cnt, cnt))

    def dev_limma_w_rss(self, A: int, Wt, aw, ld: int, rows: int, n: int, Q: int, use, p: int, nfit: int, G: int, seed, rss: int):
        """plaidhip_dev_limma_w_rss on device pointers: the weighted rss [nfit][rows] at G [nfit (p + 1)][rows]"""
        check(self.lib.plaidhip_dev_limma_w_rss(self.handle, A, Wt, aw, ld, rows, n, Q, use, p, nfit, G, seed, rss))

    def dev_row_design_effects(self, A: int, ld: int, rows: int, n: int, Q: int, use, invn: int, p: int, nfit: int, seed, E: int):
        """plaidhip_dev_row_design_effects on device pointers: E [nfit (p + 1)][rows]; use and seed may be None"""
        check(self.lib.plaidhip_dev_row_design_effects(self.handle, A, ld, rows, n, Q, use, invn, p, nfit, seed, E))

    def dev_row_design_rss(self, A: int, ld: int, rows: int, n: int, Q: int, use, p: int, nfit: int, E: int, seed, rss: int):
        """plaidhip_dev_row_design_rss on device pointers: rss [nfit][rows] at the effects E of all samples"""
        check(self.lib.plaidhip_dev_row_design_rss(self.handle, A, ld, rows, n, Q, use, p, nfit, E, seed, rss))

    def camera(self, X, design, Gp, Gi, use=None, contrasts=None, inter_gene_cor=0.01, allow_neg_cor=False):
        """plaidhip_camera: limma's competitive set test of the sets (Gp, Gi, aligned to the rows of X) for the gene statistics
        plaid.limma gives on X (genes x samples) with the designs, `use` and contrasts of Context.limma.  inter_gene_cor: the
        fixed correlation (limma's default 0.01), or None to estimate every set's variance inflation factor from the
        residuals.  (out sets x 8 x q x nfit in CAMERA_COLUMNS, hyper nfit x 6 in CAMERA_HYPER)"""
        return _camera(self.lib.plaidhip_camera, (self.handle,), X, design, Gp, Gi, use, contrasts, inter_gene_cor, allow_neg_cor)

    def fry(self, X, design, Gp, Gi, use=None, contrasts=None, standardize="posterior.sd"):
        """plaidhip_fry: limma's self-contained set test fry of the sets (Gp, Gi, aligned to the rows of X), as
        Context.camera takes its operands.  Returns (out, hyper): sets x 7 x q x nfit (FRY_COLUMNS) and nfit x 7 (FRY_HYPER)."""
        return _fry(self.lib.plaidhip_fry, (self.handle,), X, design, Gp, Gi, use, contrasts, standardize)

    def roast(self, X, design, Gp, Gi, use=None, contrasts=None, set_statistic="mean50", nrot=1999, seed=1, zscore="hill",
              midp=True, rotations=None):
        """plaidhip_roast: limma's rotation set test with sampled rotations of the sets (Gp, Gi, aligned to the rows of X), as
        Context.fry takes its operands.  Returns (out, hyper): sets x 8 x q x nfit (ROAST_COLUMNS), nfit x 7 (ROAST_HYPER)."""
        return _roast(self.lib.plaidhip_roast, (self.handle,), X, design, Gp, Gi, use, contrasts, set_statistic, nrot, seed,
                      zscore, midp, rotations)

    def romer(self, X, design, Gp, Gi, use=None, contrasts=None, set_statistic="mean", nrot=9999, seed=1, shrink_resid=True,
              shrink=None, rotations=None):
        """plaidhip_romer: limma's rotation GSEA on the ranks of the rotated moderated t of the sets (Gp, Gi, aligned to the rows
        of X), as Context.roast takes its operands.  Returns (out, hyper): sets x 7 x q x nfit (ROMER_COLUMNS), nfit x (8 + q)."""
        return _romer(self.lib.plaidhip_romer, (self.handle,), X, design, Gp, Gi, use, contrasts, set_statistic, nrot, seed,
                      shrink_resid, shrink, rotations)

    def dev_romer_keys(self, Z: int, rows: int, uidx: int, U: int, ldu: int, set_statistic: int, nrot: int, chunk: int, Ka: int,
                       Kb, Kc: int, flag):
        """plaidhip_dev_romer_keys on device pointers: the keys of the universe's rotated t as columns [rotation][ldu]"""
        check(self.lib.plaidhip_dev_romer_keys(self.handle, Z, rows, uidx, U, ldu, set_statistic, nrot, chunk, Ka, Kb, Kc, flag))

    def dev_romer_sides(self, Ra: int, Rb, Rc: int, ldu: int, U: int, Gp: int, Gi: int, m: int, set_statistic: int, nrot: int,
                        chunk: int, stat, obs, cnt):
        """plaidhip_dev_romer_sides on device pointers, from the average ranks (doubles) of the key matrices: the three int64
        sides (m x nrot x 3) and / or the counts against obs"""
        check(self.lib.plaidhip_dev_romer_sides(self.handle, Ra, Rb, Rc, ldu, U, Gp, Gi, m, set_statistic, nrot, chunk, stat, obs,
                                                cnt))

    def dev_roast_rotate(self, Rz: int, ldz: int, rows: int, n: int, beta: int, rss: int, W: int, ldw: int, nrot: int, d: float,
                         df0: float, s02: float, zscore: int, chunk: int, Z: int):
        """plaidhip_dev_roast_rotate on device pointers: z of every (gene, rotation) as [tile of 64][rows][64]"""
        check(self.lib.plaidhip_dev_roast_rotate(self.handle, Rz, ldz, rows, n, beta, rss, W, ldw, nrot, d, df0, s02, zscore,
                                                 chunk, Z))

    def dev_roast_stats(self, Z: int, rows: int, Gp: int, Gi: int, m: int, set_statistic: int, nrot: int, stat, obs, cnt):
        """plaidhip_dev_roast_stats on device pointers: the four sides (m x nrot x 4) and / or the counts against obs"""
        check(self.lib.plaidhip_dev_roast_stats(self.handle, Z, rows, Gp, Gi, m, set_statistic, nrot, stat, obs, cnt))

    def dev_fry_residuals(self, A: int, ld: int, rows: int, n: int, Q: int, use, p: int, nfit: int, fit: int, E: int, cg: int,
                          Z: int, ldz: int):
        """plaidhip_dev_fry_residuals on device pointers: dev_camera_residuals with the divisors cg ([nfit][rows])"""
        check(self.lib.plaidhip_dev_fry_residuals(self.handle, A, ld, rows, n, Q, use, p, nfit, fit, E, cg, Z, ldz))

    def dev_fry_residual_effects(self, Z: int, ldz: int, rows: int, n: int, Q2: int, use, d: int, seed, rho: int):
        """plaidhip_dev_fry_residual_effects on device pointers: rho ([d + 1][rows], the last row unused) = seed + Z Q2"""
        check(self.lib.plaidhip_dev_fry_residual_effects(self.handle, Z, ldz, rows, n, Q2, use, d, seed, rho))

    def dev_fry_gram(self, rho: int, e: int, rows: int, d: int, q: int, Gp: int, Gi: int, m: int, Cm: int, b: int, a: int,
                     tr: int, fro: int):
        """plaidhip_dev_fry_gram on device pointers: C (m x d x d), b (m x q x d), a, tr, fro (m x q) of every set"""
        check(self.lib.plaidhip_dev_fry_gram(self.handle, rho, e, rows, d, q, Gp, Gi, m, Cm, b, a, tr, fro))

    def dev_fry_eigen(self, M: int, dim: int, nprob: int, Dk: int, lam1: int, lamD: int, sweeps: int, conv: int):
        """plaidhip_dev_fry_eigen on device pointers: the largest and the Dk-th largest eigenvalue of nprob matrices"""
        check(self.lib.plaidhip_dev_fry_eigen(self.handle, M, dim, nprob, Dk, lam1, lamD, sweeps, conv))

    def dev_camera_residuals(self, A: int, ld: int, rows: int, n: int, Q: int, use, p: int, nfit: int, fit: int, E: int, rss: int,
                             d: float, Z: int, ldz: int):
        """plaidhip_dev_camera_residuals on device pointers: Z (rows x n, leading dimension ldz) of fit `fit` (from 0) at the
        effects E and the residual sums of squares rss of all samples; use may be None"""
        check(self.lib.plaidhip_dev_camera_residuals(self.handle, A, ld, rows, n, Q, use, p, nfit, fit, E, rss, float(d), Z, ldz))

    def dev_camera_sumsq(self, T: int, ldt: int, m: int, n: int, seed, out: int):
        """plaidhip_dev_camera_sumsq on device pointers: out[s] = seed[s] + the sums over the columns of T[s, c]^2 in the
        pinned block order; seed may be None"""
        check(self.lib.plaidhip_dev_camera_sumsq(self.handle, T, ldt, m, n, seed, out))

    def fisher(self, sig, Gp, Gi, overlap=False):
        """plaidhip_fisher: over-representation tests of the columns of sig (genes x lists of -1 / 0 / +1) against the sets:
        (out, tot) -- sets x 12 x lists (FISHER_COLUMNS) and the 2 x lists totals nUp, nDn; with overlap also (ov_len, ov_idx),
        the rows of every set with sig != 0, in the set's member order"""
        return _fisher(self.lib.plaidhip_fisher, (self.handle,), sig, Gp, Gi, overlap)

    def rankcor(self, stat, Gp, Gi, use_rank=True, ties="average"):
        """plaidhip_rankcor: the correlation of the columns of stat (genes x lists; NaN: the gene takes no part in the list),
        or of their ranks, with every set's membership: (out, tot) -- sets x 5 x lists (RANKCOR_COLUMNS) and the lists'
        universe sizes n"""
        return _rankcor(self.lib.plaidhip_rankcor, (self.handle,), stat, Gp, Gi, use_rank, ties)

    def plage(self, X, Gp, Gi, tol=PLAGE_TOL, maxit=1000, loadings=False):
        """plaidhip_plage / plaidhip_plage_csc: PLAGE (the first right singular vector of every set's standardized block,
        oriented as include/plaidhip.h pins it); X dense or scipy CSC.  (S, info[, loadings]): sets x samples, sets x 6
        (PLAGE_COLUMNS), and the Gp[m] loadings"""
        sparse = _is_sparse(X)
        fn = self.lib.plaidhip_plage_csc if sparse else self.lib.plaidhip_plage
        return _plage(fn, (self.handle,), X, Gp, Gi, tol, maxit, loadings, csc=sparse)

    def zscore(self, X, Gp, Gi):
        """plaidhip_zscore / plaidhip_zscore_csc: the combined z-score of every set; X dense or scipy CSC.  (S, size)"""
        sparse = _is_sparse(X)
        fn = self.lib.plaidhip_zscore_csc if sparse else self.lib.plaidhip_zscore
        return _zscore(fn, (self.handle,), X, Gp, Gi, csc=sparse)

    def gsea_permutations(self, g: int, nperm: int, seed=1) -> np.ndarray:
        """plaidhip_gsea_permutations: the genes x nperm int32 placements plaidhip_gsea generates from `seed`"""
        P = np.empty((int(g), int(nperm)), dtype=np.int32, order="F")
        check(self.lib.plaidhip_gsea_permutations(self.handle, int(g), int(nperm), int(seed) & (2**64 - 1), _np_ptr(P)))
        return P

    def dev_truncated_ranks(self, X: int, ldx: int, g: int, n: int, mode, T: int, R_scratch: int, colnan: int, counts: int,
                            Wp: int, Wi: int, Wx: int, capacity: int):
        check(self.lib.plaidhip_dev_truncated_ranks_f64(self.handle, X, ldx, g, n, TRUNC_MODE[mode], int(T), R_scratch, colnan,
                                                        counts, Wp, Wi, Wx, int(capacity)))

    def dev_truncated_ranks_csc(self, Xp: int, Xi: int, Xx: int, g: int, n: int, max_col_nnz: int, nnz: int, mode, T: int,
                                scratch: int, colnan: int, counts: int, u0: int, Wp: int, Wi: int, Wx: int, capacity: int):
        check(self.lib.plaidhip_dev_truncated_ranks_csc_f64(self.handle, Xp, Xi, Xx, g, n, max_col_nnz, nnz, TRUNC_MODE[mode],
                                                            int(T), scratch, colnan, counts, u0, Wp, Wi, Wx, int(capacity)))

    def gsva(self, X, Gp, Gi, tau=0.0, rowtf="z"):
        return self._host("gsva", _as_f64_fortran(X), Gp, Gi, float(tau), _rowtf(rowtf), dense=True)

    def gsva_csc(self, Xp, Xi, Xx, g, Gp, Gi, tau=0.0, rowtf="z"):
        """plaidhip_gsva_csc: replaid.gsva on the slots of a g x n CSC matrix (no dense X on the host)"""
        return self._host("gsva_csc", _slots(Xp, Xi, Xx, g), Gp, Gi, float(tau), _rowtf(rowtf))

    def plaid_test(self, X, y, Gp, Gi, gsetX=None, tests=7, metap_method=0):
        """plaidhip_plaid_test: returns sets x 6 (gsetFC, p.one, p.two, p.lm, p.meta, q.meta), G's column order"""
        return _plaid_test(self.lib.plaidhip_plaid_test, (self.handle,), _as_f64_fortran(X), y, Gp, Gi, gsetX, tests,
                           metap_method, dense=True)

    def plaid_test_csc(self, Xp, Xi, Xx, g, y, Gp, Gi, gsetX=None, tests=7, metap_method=0):
        """plaidhip_plaid_test_csc: Context.plaid_test on the slots of a g x n CSC matrix"""
        return _plaid_test(self.lib.plaidhip_plaid_test_csc, (self.handle,), _slots(Xp, Xi, Xx, g), y, Gp, Gi, gsetX, tests,
                           metap_method)

    def plaid_test_contrasts(self, X, Y, Gp, Gi, gsetX=None, tests=7, metap_method=0):
        """plaidhip_plaid_test_contrasts: Y n x C (0, 1, NaN or -1: the sample takes no part).  Returns sets x 6 x C,
        [:, :, j] = plaid_test on the samples of contrast j, with the scores of all samples"""
        return _plaid_test_contrasts(self.lib.plaidhip_plaid_test_contrasts, (self.handle,), _as_f64_fortran(X), Y, Gp, Gi,
                                     gsetX, tests, metap_method, dense=True)

    def plaid_test_contrasts_csc(self, Xp, Xi, Xx, g, Y, Gp, Gi, gsetX=None, tests=7, metap_method=0):
        """plaidhip_plaid_test_contrasts_csc: Context.plaid_test_contrasts on the slots of a g x n CSC matrix"""
        return _plaid_test_contrasts(self.lib.plaidhip_plaid_test_contrasts_csc, (self.handle,), _slots(Xp, Xi, Xx, g), Y, Gp,
                                     Gi, gsetX, tests, metap_method)


def plaid_test_finish(g, Gp, T, tot1, tot2, SM, n0, n1, tests=7, metap_method=0, lib=None):
    """plaidhip_plaid_test_finish (host only): the p-values, effect sizes, meta-p and FDR of plaid.test from the reduced
    statistics -- T (2, m) per-set sums of fc and fc^2, tot1 / tot2 their sums over all genes, SM (4, m) group means and
    sums of squared deviations of the score rows (None without "lm").  Returns sets x 6 like Context.plaid_test."""
    from ._lib import load
    lib = lib or load()
    Gp = _as_i32(Gp)
    m = len(Gp) - 1
    T = np.ascontiguousarray(T, dtype=np.float64)
    if T.shape != (2, m):
        raise ValueError("T must be (2, sets)")
    if SM is not None:
        SM = np.ascontiguousarray(SM, dtype=np.float64)
        if SM.shape != (4, m):
            raise ValueError("SM must be (4, sets)")
    out = np.empty((m, 6), dtype=np.float64, order="F")
    check(lib.plaidhip_plaid_test_finish(int(g), m, _np_ptr(Gp), _np_ptr(T), float(tot1), float(tot2),
                                         _np_ptr(SM) if SM is not None else None, int(n0), int(n1), int(tests),
                                         int(metap_method), _np_ptr(out)))
    return out


_default_ctx: Context | None = None


def default_context() -> Context:
    """Process-wide context on device LOCAL_RANK (or 0), private stream."""
    global _default_ctx
    if _default_ctx is None:
        import os
        _default_ctx = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _default_ctx


# ---- several GPUs from one host process (plaidhip_*_multi: a host thread per device, no RCCL) ------------------
def shard_bounds(n: int, ndev: int, k: int):
    """columns [lo, hi) of shard k of n sample columns over ndev devices (needs no device)"""
    lo, hi = C.c_int64(0), C.c_int64(0)
    check(_lib.load().plaidhip_shard_bounds(int(n), int(ndev), int(k), C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def _multi(name, devices):
    """(plaidhip_<name>_multi, its head): devices an int (devices 0 .. n-1) or a list of ordinals"""
    if devices is None:
        raise ValueError("devices: a list of device ordinals or an int (the first ndev devices)")
    fn = getattr(_lib.load(), f"plaidhip_{name}_multi")
    if isinstance(devices, int):
        return fn, (None, int(devices))
    d = np.ascontiguousarray(devices, dtype=np.int32)
    return fn, (d.ctypes.data_as(C.c_void_p), len(d))   # (the pointer object keeps d alive)


def plaid_multi(X, Gp, Gi, stat="mean", normalize=True, devices=1) -> np.ndarray:
    """plaid() with the sample columns sharded over `devices` (an int: devices 0 .. n-1, or a list of ordinals)"""
    return _score(*_multi("plaid", devices), X, Gp, Gi, STAT[stat], int(bool(normalize)))


def sing_multi(X, Gp, Gi, devices=1) -> np.ndarray:
    return _score(*_multi("sing", devices), _as_f64_fortran(X), Gp, Gi, dense=True)


def ssgsea_multi(X, Gp, Gi, alpha=0.0, devices=1) -> np.ndarray:
    return _score(*_multi("ssgsea", devices), X, Gp, Gi, float(alpha))


def ssgsea_exact_multi(X, Gp, Gi, alpha=0.25, scale=True, norm=False, devices=1, single=True) -> np.ndarray:
    """replaid.ssgsea.exact (Context.ssgsea_exact, either `single`) with the sample columns sharded over `devices`"""
    return _score(*_multi("ssgsea_exact" if single else "ssgsea_exact_ks", devices), X, Gp, Gi, float(alpha), int(bool(scale)),
                  int(bool(norm)))


def gsva_exact_multi(X, Gp, Gi, tau=1.0, rowtf="z", max_diff=True, devices=1) -> np.ndarray:
    """replaid.gsva.exact (Context.gsva_exact) with the sample columns sharded over `devices`; "ecdf" ranks all samples
    of a gene together and is refused over more than one device; "gauss" sends all of X to every device, which computes
    the kernel CDF estimate of its own columns (the one-device bits)"""
    args = check_gsva_exact_args(tau, rowtf)
    return _score(*_multi("gsva_exact", devices), X, Gp, Gi, *args, int(bool(max_diff)))


def sing_exact_multi(X, Gp, Gi, Dp=None, Di=None, center=True, dispersion=True, devices=1) -> dict:
    """replaid.sing.exact (Context.sing_exact) with the sample columns sharded over `devices`: the one-device bits"""
    return _sing_exact_call(*_multi("sing_exact", devices), X, Gp, Gi, Dp, Di, center, dispersion)


def ucell_exact_multi(X, Gp, Gi, Dp=None, Di=None, max_rank=1500, w_neg=1.0, k_full=None, k_full_down=None, devices=1) -> dict:
    """replaid.ucell.exact (Context.ucell_exact) with the sample columns sharded over `devices`: the one-device bits"""
    return _ucell_exact_call(*_multi("ucell_exact", devices), X, Gp, Gi, Dp, Di, max_rank, w_neg, k_full, k_full_down)


def aucell_exact_multi(X, Gp, Gi, auc_max_rank, devices=1) -> np.ndarray:
    """replaid.aucell.exact (Context.aucell_exact) with the sample columns sharded over `devices`: the one-device bits"""
    return _score(*_multi("aucell_exact", devices), X, Gp, Gi, float(auc_max_rank))


def ucell_multi(X, Gp, Gi, k_full, rmax=1500.0, devices=1) -> np.ndarray:
    """replaid.ucell (Context.ucell) with the sample columns sharded over `devices`"""
    kf = np.ascontiguousarray(k_full, dtype=np.float64)
    return _score(*_multi("ucell", devices), X, Gp, Gi, _np_ptr(kf), float(rmax))


def aucell_multi(X, Gp, Gi, auc_max_rank, devices=1) -> np.ndarray:
    """replaid.aucell (Context.aucell) with the sample columns sharded over `devices`"""
    return _score(*_multi("aucell", devices), X, Gp, Gi, float(auc_max_rank))


def scse_multi(X, Gp, Gi, remove_log2=None, score_mean=False, devices=1):
    """replaid.scse (Context.scse) with the sample columns sharded over `devices`: (S, removed_log2), the second
    telling whether the 2 ** x transform ran (removeLog2 = NULL is decided once, for the whole matrix)"""
    return _scse(*_multi("scse", devices), X, Gp, Gi, remove_log2, score_mean)


def gsva_multi(X, Gp, Gi, tau=0.0, rowtf="z", devices=1) -> np.ndarray:
    """replaid.gsva (Context.gsva / gsva_csc) with the sample columns sharded over `devices`; rowtf "z" only -- "ecdf"
    ranks all samples of a gene together and is refused (score it on one device)"""
    tf = _rowtf(rowtf)
    return _score(*_multi("gsva", devices), X, Gp, Gi, float(tau), tf)


def plaid_test_multi(X, y, Gp, Gi, gsetX=None, tests=7, metap_method=0, devices=1) -> np.ndarray:
    """plaid.test (Context.plaid_test / plaid_test_csc) with the sample columns sharded over `devices`; X dense or scipy
    CSC.  The scores stay on the devices: only per-gene and per-set sums cross between them.  Returns sets x 6 (gsetFC,
    p.one, p.two, p.lm, p.meta, q.meta) in G's column order; dense X gives the single-device result bit for bit."""
    return _plaid_test(*_multi("plaid_test", devices), X, y, Gp, Gi, gsetX, tests, metap_method)


def plaid_test_contrasts_multi(X, Y, Gp, Gi, gsetX=None, tests=7, metap_method=0, devices=1) -> np.ndarray:
    """plaid.test.contrasts (Context.plaid_test_contrasts / _csc) with the sample columns sharded over `devices`, as
    plaid_test_multi; sets x 6 x C, dense X the single-device result bit for bit"""
    return _plaid_test_contrasts(*_multi("plaid_test_contrasts", devices), X, Y, Gp, Gi, gsetX, tests, metap_method)


def gsea_multi(stat, weight, Gp, Gi, perm=None, nperm=1000, seed=1, null=False, devices=1, score_type="std", leading_edge=False):
    """plaid.gsea (Context.gsea) with the permutation blocks shared out over `devices`: the one-device bits"""
    if gsea_score_type(score_type) == 0 and not leading_edge:
        return _gsea(*_multi("gsea", devices), stat, weight, Gp, Gi, perm, nperm, seed, null)
    return _gsea(*_multi("gsea_scored", devices), stat, weight, Gp, Gi, perm, nperm, seed, null, score_type, leading_edge)


def gsea_multilevel_multi(stat, weight, Gp, Gi, perm=None, nperm=1000, seed=1, null=False, devices=1, score_type="std",
                          leading_edge=False, sample_size=101, sweeps=4, eps=1e-50, ml_min=10):
    """plaid.gsea with multilevel p-values (Context.gsea_multilevel), the permutation blocks and the rulers shared out over
    `devices`: the one-device bits"""
    return _gsea_multilevel(*_multi("gsea_multilevel", devices), stat, weight, Gp, Gi, perm, nperm, seed, null, score_type,
                            leading_edge, sample_size, sweeps, eps, ml_min)


def fisher_multi(sig, Gp, Gi, overlap=False, devices=1):
    """plaid.fisher (Context.fisher) with the lists shared out over `devices`: the one-device bits"""
    return _fisher(*_multi("fisher", devices), sig, Gp, Gi, overlap)


def rankcor_multi(stat, Gp, Gi, use_rank=True, ties="average", devices=1):
    """plaid.rankcor (Context.rankcor) with the lists shared out over `devices`: the one-device bits"""
    return _rankcor(*_multi("rankcor", devices), stat, Gp, Gi, use_rank, ties)


def plage_multi(X, Gp, Gi, tol=PLAGE_TOL, maxit=1000, loadings=False, devices=1):
    """replaid.plage (Context.plage) with the sample columns shared out over `devices`; every device takes all of X and
    forms every set's eigenvector: the one-device bits"""
    return _plage(*_multi("plage", devices), X, Gp, Gi, tol, maxit, loadings)


def zscore_multi(X, Gp, Gi, devices=1):
    """replaid.zscore (Context.zscore) with the sample columns shared out over `devices`: the one-device bits"""
    return _zscore(*_multi("zscore", devices), X, Gp, Gi)


def fry_multi(X, design, Gp, Gi, use=None, contrasts=None, standardize="posterior.sd", devices=1):
    """plaid.fry (Context.fry) with the sample columns sharded over `devices`: the one-device bits"""
    return _fry(*_multi("fry", devices), X, design, Gp, Gi, use, contrasts, standardize)


def roast_multi(X, design, Gp, Gi, use=None, contrasts=None, set_statistic="mean50", nrot=1999, seed=1, zscore="hill", midp=True,
                rotations=None, devices=1):
    """plaid.roast (Context.roast) with the fit's sample columns sharded over `devices`: the one-device bits"""
    return _roast(*_multi("roast", devices), X, design, Gp, Gi, use, contrasts, set_statistic, nrot, seed, zscore, midp,
                  rotations)


def romer_multi(X, design, Gp, Gi, use=None, contrasts=None, set_statistic="mean", nrot=9999, seed=1, shrink_resid=True,
                shrink=None, rotations=None, devices=1):
    """plaid.romer (Context.romer) with the rotation tiles dealt to `devices`: the one-device bits"""
    return _romer(*_multi("romer", devices), X, design, Gp, Gi, use, contrasts, set_statistic, nrot, seed, shrink_resid, shrink,
                  rotations)


def camera_multi(X, design, Gp, Gi, use=None, contrasts=None, inter_gene_cor=0.01, allow_neg_cor=False, devices=1):
    """plaid.camera (Context.camera) with the sample columns sharded over `devices`: the one-device bits"""
    return _camera(*_multi("camera", devices), X, design, Gp, Gi, use, contrasts, inter_gene_cor, allow_neg_cor)


def limma_multi(A, design, use=None, contrasts=None, devices=1, na="propagate", max_na=0.2, weights=None):
    """plaid.limma (Context.limma) with the sample columns sharded over `devices`: the one-device bits.  Returns (out, hyper),
    or with na = "fit" or weights (out, hyper nfit x 5, dfres rows x nfit) as Context.limma does"""
    fn, head = _multi("limma", devices)
    return _limma_any(fn, _multi("limma_na", devices)[0], head, A, design, use, contrasts, na, max_na, weights,
                      _multi("limma_w", devices)[0] if weights is not None else None)


def voom_multi(counts, design, lib_size=None, span=0.5, devices=1):
    """plaid.voom (Context.voom) with the sample columns sharded over `devices`: the one-device bits"""
    return _voom(*_multi("voom", devices), counts, design, lib_size, span)


def multi_finalize():
    check(_lib.load().plaidhip_multi_finalize())
