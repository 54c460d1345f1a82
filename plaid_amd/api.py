"""Host-side mirror of the reference's R API for the scoring hot path.

Same function names (dots -> underscores), argument meaning, defaults, dimnames and error
behaviour as R/plaid.R; the BODIES call the HIP library through the C ABI
(include/plaidhip.h).  There is no CPU compute path in here: gene-name alignment and
dimnames handling are host glue, everything numeric runs on the MI355X.
"""
from __future__ import annotations

import sys

import numpy as np
import scipy.sparse as sp

from ._lib import EUNSUPPORTED, PlaidHipError
from .engine import Context, default_context
from .gmt import GmtList, gmt2mat
from .matrix import NamedMatrix, as_named

INT_MAX = 2147483647  # .Machine$integer.max
_TIES = ("average", "min", "max", "first", "last", "dense", "random")   # what matrixStats::colRanks takes


def _message(txt: str):
    print(txt, file=sys.stderr)   # R message()


def _first_pos(names):
    pos = {}
    for k, nm in enumerate(names):
        pos.setdefault(nm, k)
    return pos


def aligned_pattern(X: NamedMatrix, matG: NamedMatrix):
    """Gene alignment + binarisation of R/plaid.R:65-73 without copying X:
    gg = intersect(rownames(X), rownames(matG)); G = 1*(matG[gg,] != 0), returned as a CSC
    pattern (Gp, Gi) whose row indices address X's rows.  None when nothing overlaps."""
    posx = _first_pos(X.rownames)
    G = sp.csc_matrix(matG.values)
    g2x = np.full(G.shape[0], -1, dtype=np.int64)
    seen = set()
    for k, nm in enumerate(matG.rownames):
        if nm in seen:
            continue                      # matG[gg,] picks the first row of that name
        seen.add(nm)
        r = posx.get(nm)
        if r is not None:
            g2x[k] = r
    if not np.any(g2x >= 0):
        return None
    new_idx = g2x[G.indices]
    keep = (new_idx >= 0) & (G.data != 0)
    m = G.shape[1]
    col = np.repeat(np.arange(m, dtype=np.int64), np.diff(G.indptr))
    counts = np.bincount(col[keep], minlength=m)
    Gp = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(counts, out=Gp[1:])
    if Gp[-1] > INT_MAX:
        raise PlaidHipError(EUNSUPPORTED, "membership matrix has more than 2^31-1 entries")
    return Gp.astype(np.int32), new_idx[keep].astype(np.int32)


def _auto_chunk(ncol_x: int) -> int:
    return int(np.round(0.8 * INT_MAX / max(ncol_x, 1)))     # R/plaid.R:103-104


def plaid(X, matG, stats=("mean", "sum"), chunk=None, normalize=True, ctx: Context | None = None):
    """plaid(), R/plaid.R:60-87.  Returns a NamedMatrix (sets x samples) or None with a
    message when no features overlap (:66-69)."""
    stats = stats if isinstance(stats, str) else stats[0]     # :62
    if stats not in ("mean", "sum"):
        raise ValueError("stats must be 'mean' or 'sum'")
    X, matG = as_named(X), as_named(matG)
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    Gp, Gi = pat
    ctx = ctx or default_context()
    g, n = X.shape
    m = matG.shape[1]
    auto = _auto_chunk(m)                                     # plaid passes chunk=NULL (:80)
    if n < auto:
        S = _crossprod_block(ctx, X, 0, n, Gp, Gi, stats, normalize)
    else:
        _message(f"[chunked_crossprod] chunked compute: chunk = {auto}")
        S = np.empty((m, n), dtype=np.float64, order="F")
        for j0 in range(0, n, auto):                          # :115-119
            j1 = min(n, j0 + auto)
            S[:, j0:j1] = _crossprod_block(ctx, X, j0, j1, Gp, Gi, stats, False)
        if normalize:
            S, _ = ctx.normalize_medians(S)                   # :83
    return NamedMatrix(S, matG.colnames, X.colnames)


def _crossprod_block(ctx, X: NamedMatrix, j0, j1, Gp, Gi, stats, normalize):
    if X.is_sparse:
        V = X.values[:, j0:j1] if (j0, j1) != (0, X.shape[1]) else X.values
        return ctx.plaid_csc(V.indptr, V.indices, V.data, X.shape[0], Gp, Gi, stats, normalize)
    return ctx.plaid_dense(X.values[:, j0:j1], Gp, Gi, stats, normalize)


def chunked_crossprod(x, y, chunk=None, ctx: Context | None = None):
    """chunked_crossprod(), R/plaid.R:100-123: t(x) %*% y, `x` genes x sets, `y` genes x samples with the same rows.
    A binary `x`, optionally column-scaled as plaid() builds it (:73-77), takes the scheduled membership kernels; an
    `x` whose stored values differ inside a column (weighted or signed sets) takes the general sparse kernel
    (plaidhip_crossprod_weighted_*).  Both run on the device; there is no host fallback."""
    x, y = as_named(x), as_named(y)
    if x.shape[0] != y.shape[0]:
        raise ValueError("non-conformable arguments")
    G = sp.csc_matrix(x.values)
    if not G.has_sorted_indices:
        G = G.sorted_indices()                                 # (a copy: the caller's matrix is not touched)
    m = G.shape[1]
    ctx = ctx or default_context()
    n = y.shape[1]
    if chunk is None or chunk < 0:
        chunk = _auto_chunk(m)
    scale = np.ones(m)
    nz = G.data != 0
    col = np.repeat(np.arange(m), np.diff(G.indptr))
    weighted = False
    if nz.any():
        vmin = np.full(m, np.inf)
        vmax = np.full(m, -np.inf)
        np.minimum.at(vmin, col[nz], G.data[nz])
        np.maximum.at(vmax, col[nz], G.data[nz])
        has = np.isfinite(vmin) & np.isfinite(vmax)
        # NaN / Inf weights or different values inside a column: not a (scaled) membership pattern
        weighted = bool(np.any(vmin[has] != vmax[has])) or not np.all(np.isfinite(G.data[nz]))
        if not weighted:
            scale[has] = vmin[has]
    if weighted:
        Wp, Wi, Wx = G.indptr.astype(np.int32), G.indices.astype(np.int32), G.data.astype(np.float64)
        g = x.shape[0]

        def block(j0, j1):
            if y.is_sparse:
                V = sp.csc_matrix(y.values[:, j0:j1])
                return ctx.crossprod_weighted(Wp, Wi, Wx, g, Yp=V.indptr, Yi=V.indices, Yx=V.data)
            return ctx.crossprod_weighted(Wp, Wi, Wx, g, Y=y.values[:, j0:j1])
    else:
        counts = np.bincount(col[nz], minlength=m)
        Gp = np.zeros(m + 1, dtype=np.int64)
        np.cumsum(counts, out=Gp[1:])
        Gp, Gi = Gp.astype(np.int32), G.indices[nz].astype(np.int32)

        def block(j0, j1):
            return _crossprod_block(ctx, y, j0, j1, Gp, Gi, "sum", False)
    if n < chunk:
        S = block(0, n)
    else:
        _message(f"[chunked_crossprod] chunked compute: chunk = {chunk}")
        S = np.empty((m, n), dtype=np.float64, order="F")
        for j0 in range(0, n, chunk):
            j1 = min(n, j0 + chunk)
            S[:, j0:j1] = block(j0, j1)
    if not weighted:
        S *= scale[:, None]
    return NamedMatrix(S, x.colnames, y.colnames)


def normalize_medians(x, ignore_zero=None, ctx: Context | None = None):
    """normalize_medians(), R/plaid.R:554-575."""
    x = as_named(x)
    ctx = ctx or default_context()
    S, _ = ctx.normalize_medians(x.dense(), ignore_zero)
    return NamedMatrix(S, x.rownames, x.colnames)


def _check_ties(ties_method, allowed=_TIES):
    """ties.method is passed through like the reference does (R/plaid.R:614-617, 639-642); which values are legal depends on
    the function behind the branch: matrixStats::colRanks (all), base::rank (no "dense"), sparseMatrixStats::colRanks
    (max / average / min).  An illegal value raises like R's match.arg; "random" is legal in R and refused by the library
    (PLAIDHIP_EUNSUPPORTED: not a function of the input)."""
    if ties_method not in allowed:
        raise ValueError("'arg' should be one of " + ", ".join(f"\u2018{t}\u2019" for t in allowed))


def sparse_colranks(X, signed=False, ties_method="average", ctx: Context | None = None):
    """sparse_colranks(), R/plaid.R:631-650: ranks of the stored non-zeros per column; the
    sparsity pattern is kept, @x replaced."""
    _check_ties(ties_method, ("average", "first", "last", "random", "max", "min"))     # base::rank, :639-642
    X = as_named(X)
    V = sp.csc_matrix(X.values)
    ctx = ctx or default_context()
    rx = ctx.colranks_csc(V.indptr, V.data, ties_method, signed)
    R = sp.csc_matrix((rx, V.indices.copy(), V.indptr.copy()), shape=V.shape)
    return NamedMatrix(R, X.rownames, X.colnames)


def colranks(X, sparse=None, signed=False, keep_zero=False, ties_method="average",
             ctx: Context | None = None):
    """colranks(), R/plaid.R:589-623."""
    X = as_named(X)
    if sparse is None:
        sparse = X.is_sparse                                   # :595-596
    if sparse and keep_zero:
        return sparse_colranks(X, signed=signed, ties_method=ties_method, ctx=ctx)   # :600-601
    # the `sparse` ARGUMENT picks the function: sparseMatrixStats::colRanks (:603-608) or matrixStats::colRanks (:611-617)
    _check_ties(ties_method, ("max", "average", "min") if sparse else _TIES)
    ctx = ctx or default_context()
    if X.is_sparse and ties_method not in ("max", "average", "min"):
        X = NamedMatrix(X.values.toarray(), X.rownames, X.colnames)   # sparse = FALSE on a dgCMatrix: as.matrix(X), :617
    if X.is_sparse:
        # sparse without keep.zero: the reference's result is dense with the zeros ranked
        # (sparseMatrixStats::colRanks, :603-609) -- computed from the CSC arrays on the device
        V = X.values
        R = ctx.colranks_csc_dense(V.indptr, V.indices, V.data, X.shape[0], ties_method, signed)
    else:
        R = ctx.colranks_dense(X.values, ties_method, signed)                            # :612-618
    return NamedMatrix(R, X.rownames, X.colnames)


def replaid_sing(X, matG, ctx: Context | None = None):
    """replaid.sing(), R/plaid.R:213-219: min-ranks / nrow(X) - 0.5, then plaid(normalize=FALSE)."""
    X, matG = as_named(X), as_named(matG)
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    ctx = ctx or default_context()
    if X.is_sparse:                                        # the CSC slots go to the device: no dense X on the host
        V = X.values
        S = ctx.sing_csc(V.indptr, V.indices, V.data, X.shape[0], pat[0], pat[1])
    else:
        S = ctx.sing_dense(X.values, pat[0], pat[1])
    return NamedMatrix(S, matG.colnames, X.colnames)


def replaid_ssgsea(X, matG, alpha=0, ctx: Context | None = None):
    """replaid.ssgsea(), R/plaid.R:244-255: average ranks (non-zeros only for sparse X, :245 ->
    :600-601), ^(1+alpha), / global max - 0.5, then plaid(stats="mean", normalize=TRUE)."""
    X, matG = as_named(X), as_named(matG)
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    ctx = ctx or default_context()
    if X.is_sparse:
        V = X.values
        S = ctx.ssgsea_csc(V.indptr, V.indices, V.data, X.shape[0], pat[0], pat[1], float(alpha))
    else:
        S = ctx.ssgsea_dense(X.values, pat[0], pat[1], float(alpha))
    return NamedMatrix(S, matG.colnames, X.colnames)


def replaid_ssgsea_exact(X, matG, alpha=0.25, scale=True, norm=False, single=True, ctx: Context | None = None):
    """replaid.ssgsea.exact(): the original single-sample GSEA statistic (gao.ssgsea with single = TRUE) for any alpha,
    in closed form on the device (include/plaidhip.h: plaidhip_ssgsea_exact).  G is aligned to X's rows as plaid()
    aligns it; k counts the aligned members.  A dgCMatrix scores as as.matrix(X) would.  single = False: the running
    sum's value of largest magnitude (the classic GSEA enrichment score; plaidhip_ssgsea_exact_ks) instead of its sum."""
    X, matG = as_named(X), as_named(matG)
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    ctx = ctx or default_context()
    S = ctx.ssgsea_exact(X.values, pat[0], pat[1], float(alpha), scale, norm, single)
    return NamedMatrix(S, matG.colnames, X.colnames)


def _set_sizes_unaligned(matG: NamedMatrix) -> np.ndarray:
    """Matrix::colSums(matG != 0) of the matrix as given (R/plaid.R:280 does not re-align)."""
    G = sp.csc_matrix(matG.values)
    col = np.repeat(np.arange(G.shape[1]), np.diff(G.indptr))
    return np.bincount(col[G.data != 0], minlength=G.shape[1]).astype(np.float64)


def replaid_ucell(X, matG, rmax=1500, ctx: Context | None = None):
    """replaid.ucell(), R/plaid.R:276-282."""
    X, matG = as_named(X), as_named(matG)
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    ctx = ctx or default_context()
    S = ctx.ucell(X.values, pat[0], pat[1], _set_sizes_unaligned(matG), float(rmax))
    return NamedMatrix(S, matG.colnames, X.colnames)


def replaid_aucell(X, matG, aucMaxRank=None, ctx: Context | None = None):
    """replaid.aucell(), R/plaid.R:304-309; aucMaxRank defaults to ceiling(0.05 * nrow(X))."""
    X, matG = as_named(X), as_named(matG)
    if aucMaxRank is None:
        aucMaxRank = int(np.ceil(0.05 * X.shape[0]))
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    ctx = ctx or default_context()
    S = ctx.aucell(X.values, pat[0], pat[1], float(aucMaxRank))
    return NamedMatrix(S, matG.colnames, X.colnames)


def replaid_scse(X, matG, removeLog2=None, scoreMean=False, ctx: Context | None = None):
    """replaid.scse(), R/plaid.R:155-190."""
    X, matG = as_named(X), as_named(matG)
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    ctx = ctx or default_context()
    S = ctx.scse(X.values, pat[0], pat[1], removeLog2, scoreMean)
    if ctx.last_scse_removed_log2:        # R/plaid.R:163-164 (removeLog2 = NULL is decided on the device, :160-161)
        _message("[replaid.scse] Converting data to linear scale (removing log2)...")
    return NamedMatrix(S, matG.colnames, X.colnames)


def _canonical_csc(V):
    """V as a CSC matrix whose columns have sorted, distinct row indices (a dgCMatrix always does; scipy may not),
    so that its slots mean what as.matrix() means.  A copy only when V is not already so."""
    V = sp.csc_matrix(V)                                   # (shares the slots of a CSC matrix)
    if not V.has_canonical_format:
        V = V.copy()
        V.sum_duplicates()
    return V


def replaid_gsva(X, matG, tau=0, rowtf="z", ctx: Context | None = None):
    """replaid.gsva(), R/plaid.R:338-363 (row z-transform variant; the result of plaid() on the rank matrix
    carries the dimnames of matG / X)."""
    rowtf = rowtf if isinstance(rowtf, str) else rowtf[0]
    X, matG = as_named(X), as_named(matG)
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    ctx = ctx or default_context()
    if X.is_sparse:                                        # the CSC slots go to the device: no dense X on the host
        V = _canonical_csc(X.values)
        S = ctx.gsva_csc(V.indptr, V.indices, V.data, X.shape[0], pat[0], pat[1], float(tau), rowtf)
    else:
        S = ctx.gsva(X.values, pat[0], pat[1], float(tau), rowtf)
    return NamedMatrix(S, matG.colnames, X.colnames)


def replaid_gsva_exact(X, matG, tau=1, rowtf="z", max_diff=True, ctx: Context | None = None):
    """replaid.gsva.exact(): the random-walk statistic of GSVA (Haenzelmann et al. 2013; include/plaidhip.h:
    plaidhip_gsva_exact) where replaid.gsva is a mean of transformed ranks.  rowtf "z" / "ecdf" are replaid.gsva's row
    transforms, "none" takes X as it is (a caller's own per-gene CDF), "gauss" is GSVA's own default: the Gaussian kernel
    CDF estimate of every value among its gene's samples (Context.gsva_kcdf; at least 2 samples).  The genes of a sample are walked in decreasing
    order of the transformed value (ties in row order) with the weights |rank - N / 2| ^ tau; max_diff = True adds the
    walk's largest positive and negative excursion, False returns the larger one (the negative one when equal).  No
    normalize_medians; GSVA's Poisson kernel and abs.ranking are not offered.  tau and rowtf are checked before
    any device is touched."""
    from .engine import check_gsva_exact_args
    tau, _ = check_gsva_exact_args(tau, rowtf)
    rowtf = rowtf if isinstance(rowtf, str) else rowtf[0]
    X, matG = as_named(X), as_named(matG)
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    ctx = ctx or default_context()
    V = _canonical_csc(X.values) if X.is_sparse else X.values   # the CSC slots go to the device: no dense X on the host
    S = ctx.gsva_exact(V, pat[0], pat[1], tau, rowtf, max_diff)
    return NamedMatrix(S, matG.colnames, X.colnames)


def _sized_pattern(X, matG, minSize, maxSize):
    """the aligned pattern of the sets with minSize <= aligned members <= maxSize (None: no upper limit), and their names"""
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    Gp, Gi = np.asarray(pat[0]), np.asarray(pat[1])
    sizes = np.diff(Gp)
    keep = np.flatnonzero((sizes >= int(minSize)) & (sizes <= (sizes.max(initial=0) if maxSize is None else int(maxSize))))
    Gi = np.concatenate([Gi[Gp[j]:Gp[j + 1]] for j in keep]).astype(np.int32) if len(keep) else np.zeros(0, np.int32)
    Gp = np.concatenate([[0], np.cumsum(sizes[keep])]).astype(np.int32)
    return Gp, Gi, [matG.colnames[j] for j in keep]


def replaid_plage(X, matG, minSize=1, maxSize=None, tol=2.0 ** -40, maxit=1000, loadings=False, ctx: Context | None = None):
    """replaid.plage(): GSVA's method = "plage" (Tomfohr et al. 2005) -- per set the first right singular vector of the
    standardized expression block of its genes, the set's "activity" across the samples -- as pinned in include/plaidhip.h
    (plaidhip_plage).  Genes are standardized over all samples (GSVA's scale()); constant genes are left out of every set;
    a gene holding NaN or Inf makes the scores of its sets NaN.  The sign, arbitrary in LAPACK and so in GSVA, is pinned:
    the score rises when the set's genes rise on average.  X dense or sparse (scored as its dense form).  Sets with fewer
    than minSize or more than maxSize aligned members are dropped; maxSize above the cap of 4096 members is a ValueError, and
    so is a kept set above it.  tol, maxit: the stop test and the step cap of the power iteration.  Returns (scores, info):
    sets x samples, and sets x [size, lambda, explained, iterations, residual, converged]; with loadings = True also a
    dict, set -> (gene names, loadings) over the set's aligned members (0 for a dropped constant gene)."""
    from .engine import PLAGE_COLUMNS, PLAGE_MAX_SET
    if maxSize is not None and int(maxSize) > PLAGE_MAX_SET:
        raise ValueError(f"replaid.plage: maxSize = {int(maxSize)} (at most {PLAGE_MAX_SET} members)")
    if not (float(tol) > 0.0):
        raise ValueError(f"replaid.plage: tol = {tol} (a positive number)")
    if int(maxit) < 1:
        raise ValueError(f"replaid.plage: maxit = {maxit} (at least 1)")
    X, matG = as_named(X), as_named(matG)
    pat = _sized_pattern(X, matG, minSize, maxSize)
    if pat is None:
        return None
    Gp, Gi, names = pat
    if len(Gp) > 1 and int(np.diff(Gp).max()) > PLAGE_MAX_SET:
        raise ValueError(f"replaid.plage: a set of {int(np.diff(Gp).max())} members (at most {PLAGE_MAX_SET}; set maxSize)")
    ctx = ctx or default_context()
    V = _canonical_csc(X.values) if X.is_sparse else X.values
    res = ctx.plage(V, Gp, Gi, tol, maxit, loadings)
    out = (NamedMatrix(res[0], names, X.colnames), NamedMatrix(res[1], names, list(PLAGE_COLUMNS)))
    if not loadings:
        return out
    load = {nm: ([X.rownames[i] for i in Gi[Gp[j]:Gp[j + 1]]], res[2][Gp[j]:Gp[j + 1]].copy()) for j, nm in enumerate(names)}
    return out + (load,)


def replaid_zscore(X, matG, ctx: Context | None = None):
    """replaid.zscore(): GSVA's method = "zscore" (Lee et al. 2008) -- the sum of a set's standardized genes over the
    square root of their number -- as pinned in include/plaidhip.h (plaidhip_zscore).  Genes are standardized over all
    samples (GSVA's scale()); constant genes are left out of every set; a set without a kept gene scores NaN, and so does
    every set holding a gene with NaN or Inf.  X dense or sparse (scored as its dense form).  Returns sets x samples."""
    X, matG = as_named(X), as_named(matG)
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    ctx = ctx or default_context()
    V = _canonical_csc(X.values) if X.is_sparse else X.values
    S, _ = ctx.zscore(V, pat[0], pat[1])
    return NamedMatrix(S, matG.colnames, X.colnames)


def replaid_sing_exact(X, matG, matD=None, center=True, dispersion=True, ctx: Context | None = None):
    """replaid.sing.exact(): singscore's normalised score (mean rank - low) / (high - low) [- 0.5] and its dispersion, the
    MAD of the set's ranks in the sample (include/plaidhip.h: plaidhip_sing_exact), where replaid.sing returns
    mean(rank) / N - 0.5.  matD (optional): the down sets, column j pairing with column j of matG, with its own row
    names.  Returns a dict of NamedMatrix: UpScore and UpDispersion; with matD also TotalScore, DownScore,
    TotalDispersion and DownDispersion (Total = Up + Down).  dispersion = False returns the scores alone.  The arguments
    are checked before any device is touched."""
    from .engine import check_sing_exact_args
    X, matG = as_named(X), as_named(matG)
    if matD is not None:
        matD = as_named(matD)
        if matD.shape[1] != matG.shape[1]:
            raise ValueError(f"sing_exact: matD has {matD.shape[1]} columns, matG {matG.shape[1]}")
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    dpat = (None, None)
    if matD is not None:
        dpat = aligned_pattern(X, matD)
        if dpat is None:   # no down gene among X's rows: every down column is empty
            dpat = (np.zeros(matD.shape[1] + 1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    check_sing_exact_args(X.shape[0], pat[0], dpat[0], dispersion)
    ctx = ctx or default_context()
    V = _canonical_csc(X.values) if X.is_sparse else X.values   # the CSC slots go to the device: no dense X on the host
    out = ctx.sing_exact(V, pat[0], pat[1], dpat[0], dpat[1], center, dispersion)
    return {name: NamedMatrix(S, matG.colnames, X.colnames) for name, S in out.items()}


def replaid_ucell_exact(X, matG, matD=None, maxRank=1500, w_neg=1, k_full=None, impute=False, ctx: Context | None = None):
    """replaid.ucell.exact(): UCell's statistic (include/plaidhip.h: plaidhip_ucell_exact) where replaid.ucell is near exact:
    the descending average ranks truncated by UCell's rule (d <= maxRank ? d : maxRank + 1), the Mann-Whitney form in
    integers closed by one division, no median normalisation.  matD (optional): the down sets, column j pairing with column
    j of matG; TotalScore = UpScore - w_neg * DownScore, clamped at 0.  impute = True is UCell's missing_genes = "impute":
    the members of a set that X lacks count with rank maxRank + 1 (k_full = colSums(matG != 0) of the un-aligned matrix; a k_full of the caller's overrides it for the up sets).
    A sparse X is never expanded.  Returns a dict of NamedMatrix: UpScore, and with matD also TotalScore and DownScore.
    The arguments are checked before any device is touched."""
    from .engine import check_truncated_rank
    X, matG = as_named(X), as_named(matG)
    if matD is not None:
        matD = as_named(matD)
        if matD.shape[1] != matG.shape[1]:
            raise ValueError(f"ucell_exact: matD has {matD.shape[1]} columns, matG {matG.shape[1]}")
    w_neg = float(w_neg)
    if not np.isfinite(w_neg) or w_neg < 0.0:
        raise ValueError(f"ucell_exact: w_neg must be finite and >= 0 (got {w_neg:g})")
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    T = check_truncated_rank("ucell_exact", "maxRank", X.shape[0], maxRank)
    dpat = (None, None)
    if matD is not None:
        dpat = aligned_pattern(X, matD)
        if dpat is None:   # no down gene among X's rows: every down column is empty
            dpat = (np.zeros(matD.shape[1] + 1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    impute = bool(impute) or k_full is not None
    kf = (np.asarray(k_full, dtype=np.float64) if k_full is not None else _set_sizes_unaligned(matG)) if impute else None
    kd = _set_sizes_unaligned(matD) if impute and matD is not None else None
    ctx = ctx or default_context()
    V = _canonical_csc(X.values) if X.is_sparse else X.values   # the CSC slots go to the device: no dense X anywhere
    out = ctx.ucell_exact(V, pat[0], pat[1], dpat[0], dpat[1], T, w_neg, kf, kd)
    return {name: NamedMatrix(S, matG.colnames, X.colnames) for name, S in out.items()}


def replaid_aucell_exact(X, matG, aucMaxRank=None, ctx: Context | None = None):
    """replaid.aucell.exact(): AUCell's AUC (include/plaidhip.h: plaidhip_aucell_exact) where replaid.aucell is a ramp with a
    factor of 1.08: the area under the recovery curve over the first aucMaxRank - 1 positions, divided by the largest area
    a set of its size can reach.  aucMaxRank defaults to ceiling(0.05 * nrow(X)).  Ties are broken by row order (AUCell
    breaks them at random); no median normalisation.  A sparse X is never expanded.  The arguments are checked before any
    device is touched."""
    from .engine import check_truncated_rank
    X, matG = as_named(X), as_named(matG)
    if aucMaxRank is None:
        aucMaxRank = int(np.ceil(0.05 * X.shape[0]))
    pat = aligned_pattern(X, matG)
    if pat is None:
        _message("[plaid] ERROR. No overlapping features.")
        return None
    A = check_truncated_rank("aucell_exact", "aucMaxRank", X.shape[0], aucMaxRank)
    ctx = ctx or default_context()
    V = _canonical_csc(X.values) if X.is_sparse else X.values
    S = ctx.aucell_exact(V, pat[0], pat[1], A)
    return NamedMatrix(S, matG.colnames, X.colnames)


_TEST_BITS = {"one": 1, "two": 2, "lm": 4}


def _plaid_test_operands(X, G, gsetX, tests, metap_method):
    """What plaid_test and plaid_test_contrasts share before the device: G from a gmt, the tests' bit mask, the meta-p
    code, the rows of X and G aligned by name (:403-405), gsetX's rows in G's column order.
    Returns (Xs, Gp, Gi, sx, bits, mm, tests, the set names)."""
    if isinstance(G, (GmtList, dict)) or (isinstance(G, tuple) and len(G) == 2):
        _message("[plaid.test] converting gmt to sparse matrix...")           # :396-397
        G = gmt2mat(G)
    X, G = as_named(X), as_named(G)
    tests = [tests] if isinstance(tests, str) else list(tests)
    bits = 0
    for t in tests:
        if t not in _TEST_BITS:
            raise ValueError(f"unknown test {t!r}")
        bits |= _TEST_BITS[t]
    if metap_method in ("fisher", "sumlog"):
        mm = 0
    elif metap_method in ("stouffer", "sumz"):
        mm = 1
    else:
        raise ValueError("Invalid method: " + str(metap_method))              # :533
    # gg <- intersect(rownames(G), rownames(X)); X <- X[gg,]; G <- G[gg,]    (:403-405)
    posx = _first_pos(X.rownames)
    seen, grow, xrow = set(), [], []
    for k, nm in enumerate(G.rownames):
        if nm in seen:
            continue
        seen.add(nm)
        r = posx.get(nm)
        if r is not None:
            grow.append(k)
            xrow.append(r)
    Gs = sp.csc_matrix(G.values)[grow, :].tocsc()
    Gs.sort_indices()
    keep = Gs.data != 0
    counts = np.bincount(np.repeat(np.arange(Gs.shape[1]), np.diff(Gs.indptr))[keep], minlength=Gs.shape[1])
    Gp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    Gi = Gs.indices[keep].astype(np.int32)
    Xv = X.values
    if sp.issparse(Xv):
        Xs = sp.csc_matrix(Xv)
        if not np.array_equal(xrow, np.arange(Xs.shape[0])):
            Xs = Xs[xrow, :]                                          # X[gg, ] stays sparse
        Xs = _canonical_csc(Xs)
    else:
        Xs = np.asfortranarray(np.asarray(Xv)[xrow, :], dtype=np.float64)
    sx = None
    if gsetX is not None:
        gx = as_named(gsetX)
        if gx.rownames is not None and list(gx.rownames) != list(G.colnames):
            pos = _first_pos(gx.rownames)
            sx = np.asarray(gx.values)[[pos[nm] for nm in G.colnames], :]
        else:
            sx = np.asarray(gx.values)
    return Xs, Gp, Gi, sx, bits, mm, tests, list(G.colnames)


def _plaid_test_table(out, tests, rn, sort_by):
    """sets x 6 of the library -> the NamedMatrix plaid.test returns: the columns asked for, ordered by `sort_by` (:469-471)"""
    cols, names = [0], ["gsetFC"]
    for t, c in (("one", 1), ("two", 2), ("lm", 3)):
        if t in tests:
            cols.append(c)
            names.append("p." + t)
    cols += [4, 5]
    names += ["p.meta", "q.meta"]
    res = out[:, cols]
    rn = list(rn)
    if sort_by in names:
        o = np.argsort(res[:, names.index(sort_by)], kind="stable")       # order()
        res = res[o, :]
        rn = [rn[k] for k in o]
    return NamedMatrix(res, rn, names)


def plaid_test(X, y, G, gsetX=None, tests=("one", "two", "lm"), metap_method="fisher", sort_by="p.meta",
               ctx: Context | None = None):
    """plaid.test(), R/plaid.R:392-474: one-/two-sample t-tests of the logFC inside each set plus a Welch test
    of the single-sample scores between the two groups, combined by Fisher or Stouffer, BH-adjusted.
    The statistics are reduced on the device; with gsetX=None the scores plaid(X, G) never leave it.
    Returns a NamedMatrix (sets x [gsetFC, p.<test>..., p.meta, q.meta]) ordered by `sort_by` (:469-471)."""
    y = np.asarray(y)
    if not np.all(np.isin(np.unique(y), (0, 1))):
        raise ValueError("elements of y must be 0 or 1")                      # :394
    Xs, Gp, Gi, sx, bits, mm, tests, rn = _plaid_test_operands(X, G, gsetX, tests, metap_method)
    ctx = ctx or default_context()
    if sp.issparse(Xs):
        out = ctx.plaid_test_csc(Xs.indptr, Xs.indices, Xs.data, Xs.shape[0], y.astype(np.int32), Gp, Gi, sx, bits, mm)
    else:
        out = ctx.plaid_test(Xs, y.astype(np.int32), Gp, Gi, sx, bits, mm)
    return _plaid_test_table(out, tests, rn, sort_by)


def plaid_test_contrasts(X, Y, G, gsetX=None, tests=("one", "two", "lm"), metap_method="fisher", sort_by="p.meta",
                         ctx: Context | None = None):
    """plaid.test.contrasts(): plaid.test for every column of the contrast matrix Y (samples x contrasts; 0, 1, and NaN or
    -1 for a sample that takes no part in the contrast) in one pass over the scores.  Contrast j is
    plaid.test(X[, sel], Y[sel, j], G, gsetX = S_all[, sel]) with sel the samples of the contrast and S_all the gsetX given,
    or plaid(X, G) over all samples, computed once.  Y: a NamedMatrix (its column names name the contrasts) or an array
    (contrasts "1", "2", ...).  Returns a dict in Y's column order: contrast name -> the NamedMatrix plaid_test returns."""
    from .engine import contrast_labels
    Yn = Y if isinstance(Y, NamedMatrix) else None
    Yv = np.asarray(Yn.values if Yn is not None else Y)
    if Yv.ndim == 1:
        Yv = Yv[:, None]
    ncon = Yv.shape[1] if Yv.ndim == 2 else 0
    names = list(Yn.colnames) if Yn is not None and Yn.colnames is not None else [str(j + 1) for j in range(ncon)]
    Xs, Gp, Gi, sx, bits, mm, tests, rn = _plaid_test_operands(X, G, gsetX, tests, metap_method)
    lab = contrast_labels(Yv, Xs.shape[1])
    if not np.all(np.isin(lab, (0, 1, -1))):
        raise ValueError("elements of Y must be 0, 1 or NA")
    ctx = ctx or default_context()
    if sp.issparse(Xs):
        out = ctx.plaid_test_contrasts_csc(Xs.indptr, Xs.indices, Xs.data, Xs.shape[0], lab, Gp, Gi, sx, bits, mm)
    else:
        out = ctx.plaid_test_contrasts(Xs, lab, Gp, Gi, sx, bits, mm)
    return {nm: _plaid_test_table(out[:, :, j], tests, rn, sort_by) for j, nm in enumerate(names)}


_GSEA_NAMES = ["ES", "NES", "pval", "padj", "nMoreExtreme", "size"]


_GSEA_SCORE_TYPES = ("std", "pos", "neg")


def plaid_gsea(stats, G, nperm=1000, gseaParam=1, minSize=1, maxSize=None, seed=1, perm=None, sort_by="pval",
               ctx: Context | None = None, scoreType="std", leadingEdge=False, multilevel=False, sampleSize=101, eps=1e-50,
               sweeps=4, mlMin=10):
    """plaid.gsea(): preranked GSEA (fgsea's fgseaSimple as pinned in include/plaidhip.h) of a named
    vector of statistics, or of every column of a genes x contrasts NamedMatrix, against the sets of G (a gmt or a
    membership matrix), with a permutation null of `nperm` placements generated on the device from `seed` (or the caller's
    `perm`, genes x permutations int32 over the aligned genes).  Genes are aligned by name as plaid.test aligns them; the
    weights |stat|^gseaParam are formed here, on the host.  Sets with fewer than minSize or more than maxSize (default: the
    aligned genes - 1) aligned members are dropped.  Returns one NamedMatrix (sets x [ES, NES, pval, padj, nMoreExtreme,
    size]) ordered by `sort_by` when stats is a named vector (a dict or a pandas Series, gene -> statistic); for a
    NamedMatrix, of one column or of many, a dict, column name -> NamedMatrix, in the columns' order.  The default seed is
    plaid.gsea's in the R package, so the same call gives the same table in both.
    scoreType "pos" / "neg" scores one side of the walk (for a statistic of one sign, such as |logFC|, F or -log p).
    leadingEdge = True returns (table, edges) wherever a table is returned: edges is a list, one entry per table row in
    the table's order, of the gene names that drive the set's score, in walk order.
    multilevel = True (fgsea's multilevel reading, as pinned in include/plaidhip.h: plaidhip_gsea_multilevel) replaces the
    pval of every set that fewer than mlMin permutations matched by an adaptive multilevel splitting estimate from
    sampleSize chains (odd), `sweeps` * size proposals a stage, down to about eps; padj is over the reported pval, and the
    table gains a log2err column (the expected error of log2 pval; NaN where the permutation pval stands)."""
    if scoreType not in _GSEA_SCORE_TYPES:
        raise ValueError(f"plaid.gsea: scoreType must be one of {list(_GSEA_SCORE_TYPES)} (got {scoreType!r})")
    if isinstance(stats, dict):
        stats = NamedMatrix(np.array(list(stats.values()), dtype=np.float64), list(stats.keys()), ["stat"])
        single = True
    else:
        single = not isinstance(stats, NamedMatrix) and np.ndim(stats) == 1
        try:
            import pandas as pd
            if isinstance(stats, pd.Series):
                stats, single = NamedMatrix(stats.to_numpy(dtype=np.float64), list(stats.index), ["stat"]), True
        except ImportError:  # pragma: no cover
            pass
    if isinstance(G, (GmtList, dict)) or (isinstance(G, tuple) and len(G) == 2):
        _message("[plaid.gsea] converting gmt to sparse matrix...")
        G = gmt2mat(G)
    stats = as_named(stats)
    if sp.issparse(stats.values):
        raise ValueError("plaid.gsea: stats must be dense")
    gp = float(gseaParam)
    if not np.isfinite(gp) or gp < 0.0:
        raise ValueError(f"plaid.gsea: gseaParam must be finite and >= 0 (got {gp:g})")
    Xs, Gp, Gi, _, _, _, _, rn = _plaid_test_operands(stats, G, None, "one", "fisher")
    N = Xs.shape[0]
    sizes = np.diff(Gp)
    hi = N - 1 if maxSize is None else int(maxSize)
    keep = np.flatnonzero((sizes >= int(minSize)) & (sizes <= hi))
    Gi = np.concatenate([Gi[Gp[j]:Gp[j + 1]] for j in keep]).astype(np.int32) if len(keep) else np.zeros(0, np.int32)
    Gp = np.concatenate([[0], np.cumsum(sizes[keep])]).astype(np.int32)
    rn = [rn[j] for j in keep]
    with np.errstate(invalid="ignore"):
        W = np.ones_like(Xs) if gp == 0.0 else (np.abs(Xs) if gp == 1.0 else np.abs(Xs) ** gp)
    W = np.where(np.isfinite(W), W, 0.0)   # (a list with a NaN or an infinity is NaN by the statistic's own rule)
    ctx = ctx or default_context()
    cols = _GSEA_NAMES
    if multilevel:
        res = ctx.gsea_multilevel(Xs, W, Gp, Gi, perm=perm, nperm=nperm, seed=seed, score_type=scoreType,
                                  leading_edge=bool(leadingEdge), sample_size=sampleSize, sweeps=sweeps, eps=eps, ml_min=mlMin)
        out, ml = res[0], res[1]
        used = out[:, 4, :] < int(mlMin)                      # where pvalML is the reported pval
        out = np.concatenate([out[:, :6, :], np.where(used, ml[:, 1, :], np.nan)[:, None, :]], axis=1)
        cols = _GSEA_NAMES + ["log2err"]
        if leadingEdge:
            le_len, le_idx = res[2], res[3]
    else:
        out = ctx.gsea(Xs, W, Gp, Gi, perm=perm, nperm=nperm, seed=seed, score_type=scoreType, leading_edge=bool(leadingEdge))
        if leadingEdge:
            out, le_len, le_idx = out
    if leadingEdge:
        posx = _first_pos(stats.rownames)
        genes = [nm for nm in dict.fromkeys(as_named(G).rownames) if nm in posx]     # the aligned rows, as Gi numbers them
    res = {}
    for l, nm in enumerate(stats.colnames):
        tab, names = out[:, :len(cols), l], list(rn)
        o = np.arange(len(names))
        if sort_by in cols:
            o = np.argsort(tab[:, cols.index(sort_by)], kind="stable")       # order(): NaN last
            tab, names = tab[o, :], [names[k] for k in o]
        res[nm] = NamedMatrix(tab, names, list(cols))
        if leadingEdge:
            res[nm] = (res[nm], [[genes[r] for r in le_idx[Gp[j]:Gp[j] + le_len[j, l], l]] for j in o])
    return res[stats.colnames[0]] if single and len(res) == 1 else res


_FISHER_NAMES = ["size", "ovUp", "ovDn", "pUp", "pDn", "pAny", "padjUp", "padjDn", "padjAny", "orUp", "orDn", "orAny"]


def plaid_sig(logFC, pvalue, lfc=0.2, pcut=0.05):
    """plaid.sig(): the lists plaid.fisher takes, from gene-level results: +1 where logFC > lfc and pvalue < pcut, -1 where
    logFC < -lfc and pvalue < pcut, 0 elsewhere; a NaN in either input gives 0.  (The rule of the reference's comparison
    of enrichment methods.)  logFC and pvalue have one shape (a vector, a dict / Series, or genes x contrasts); a
    NamedMatrix, dict or Series comes back as a NamedMatrix with the same names, anything else as an int8 array.  Runs
    on the host."""
    names = None
    if isinstance(logFC, dict):
        names = (list(logFC.keys()), ["sig"])
        pvalue = [pvalue[k] for k in logFC] if isinstance(pvalue, dict) else pvalue
        logFC = list(logFC.values())
    elif isinstance(logFC, NamedMatrix):
        names = (logFC.rownames, logFC.colnames)
        logFC = logFC.values
    elif hasattr(logFC, "index") and hasattr(logFC, "to_numpy"):     # a pandas Series / DataFrame
        names = (list(logFC.index), list(getattr(logFC, "columns", ["sig"])))
        logFC = logFC.to_numpy(dtype=np.float64)
    if isinstance(pvalue, NamedMatrix):
        pvalue = pvalue.values
    elif hasattr(pvalue, "to_numpy"):
        pvalue = pvalue.to_numpy(dtype=np.float64)
    fc, pv = np.asarray(logFC, dtype=np.float64), np.asarray(pvalue, dtype=np.float64)
    if fc.shape != pv.shape:
        raise ValueError(f"plaid.sig: logFC {fc.shape} and pvalue {pv.shape} must have one shape")
    with np.errstate(invalid="ignore"):   # (a comparison with NaN is False: 0)
        hit = pv < float(pcut)
        s = (hit & (fc > float(lfc))).astype(np.int8) - (hit & (fc < -float(lfc))).astype(np.int8)
    if names is None:
        return s
    return NamedMatrix(s.reshape(len(names[0]), -1), names[0], names[1])


def plaid_fisher(sig, G, minSize=1, maxSize=None, sort_by="pAny", overlap=False, ctx: Context | None = None):
    """plaid.fisher(): over-representation analysis (Fisher's exact / hypergeometric test, upper tail, as pinned in
    include/plaidhip.h) of a named vector of -1 / 0 / +1 (gene significant down / not / up; plaid_sig makes one), or of
    every column of a genes x contrasts NamedMatrix, against the sets of G (a gmt or a membership matrix).  Genes are
    aligned by name as plaid.gsea aligns them, and the universe is the aligned rows.  Sets with fewer than minSize or more
    than maxSize (default: the aligned genes - 1) aligned members are dropped.  Returns one NamedMatrix (sets x [size, ovUp,
    ovDn, pUp, pDn, pAny, padjUp, padjDn, padjAny, orUp, orDn, orAny]) ordered by `sort_by` (stable, NaN last) when sig is a
    named vector (a dict or a pandas Series); for a NamedMatrix, of one column or of many, a dict, column name ->
    NamedMatrix, in the columns' order.  overlap = True returns (table, genes) wherever a table is returned: genes is a
    list, one entry per table row in the table's order, of (gene name, sign) for the set's members that are in the list, in
    the set's member order."""
    if isinstance(sig, dict):
        sig = NamedMatrix(np.array(list(sig.values()), dtype=np.float64), list(sig.keys()), ["sig"])
        single = True
    else:
        single = not isinstance(sig, NamedMatrix) and np.ndim(sig) == 1
        try:
            import pandas as pd
            if isinstance(sig, pd.Series):
                sig, single = NamedMatrix(sig.to_numpy(dtype=np.float64), list(sig.index), ["sig"]), True
        except ImportError:  # pragma: no cover
            pass
    if isinstance(G, (GmtList, dict)) or (isinstance(G, tuple) and len(G) == 2):
        _message("[plaid.fisher] converting gmt to sparse matrix...")
        G = gmt2mat(G)
    sig = as_named(sig)
    if sp.issparse(sig.values):
        raise ValueError("plaid.fisher: sig must be dense")
    Xs, Gp, Gi, _, _, _, _, rn = _plaid_test_operands(sig, G, None, "one", "fisher")
    N = Xs.shape[0]
    sizes = np.diff(Gp)
    hi = N - 1 if maxSize is None else int(maxSize)
    keep = np.flatnonzero((sizes >= int(minSize)) & (sizes <= hi))
    Gi = np.concatenate([Gi[Gp[j]:Gp[j + 1]] for j in keep]).astype(np.int32) if len(keep) else np.zeros(0, np.int32)
    Gp = np.concatenate([[0], np.cumsum(sizes[keep])]).astype(np.int32)
    rn = [rn[j] for j in keep]
    ctx = ctx or default_context()
    res_dev = ctx.fisher(Xs, Gp, Gi, overlap=bool(overlap))
    out = res_dev[0]
    if overlap:
        ov_len, ov_idx = res_dev[2], res_dev[3]
        posx = _first_pos(sig.rownames)
        genes = [nm for nm in dict.fromkeys(as_named(G).rownames) if nm in posx]     # the aligned rows, as Gi numbers them
    res = {}
    for l, nm in enumerate(sig.colnames):
        tab, names = out[:, :, l], list(rn)
        o = np.arange(len(names))
        if sort_by in _FISHER_NAMES:
            o = np.argsort(tab[:, _FISHER_NAMES.index(sort_by)], kind="stable")       # order(): NaN last
            tab, names = tab[o, :], [names[k] for k in o]
        res[nm] = NamedMatrix(tab, names, _FISHER_NAMES)
        if overlap:
            res[nm] = (res[nm], [[(genes[r], int(Xs[r, l])) for r in ov_idx[Gp[j]:Gp[j] + ov_len[j, l], l]] for j in o])
    return res[sig.colnames[0]] if single and len(res) == 1 else res


_RANKCOR_NAMES = ["size", "rho", "t", "p.value", "q.value"]


def plaid_rankcor(stat, G, use_rank=True, compute_p=True, ties="average", minSize=1, maxSize=None, sort_by="p.value",
                  ctx: Context | None = None):
    """plaid.rankcor(): the reference's gset.rankcor(fc, matG, compute.p = TRUE) -- the Pearson correlation of the ranks of a
    per-gene statistic (use_rank = False: of the statistic itself) with the 0/1 membership of every set of G (a gmt or a
    membership matrix), as pinned in include/plaidhip.h -- for a named vector (a dict or a pandas Series, gene ->
    statistic) or every column of a genes x lists NamedMatrix (contrasts, or samples).  A NaN leaves the gene out of that
    list alone: the ranks, the universe and the sets' sizes are taken over the list's own genes.  Genes are aligned by name
    as plaid.gsea aligns them.  ties: "average" (default), "min" or "max"; the reference's "random" is no function of the
    input and is not offered (lists without ties are the same under all of them).  Sets with fewer than minSize or more than
    maxSize (default: the aligned genes - 1) aligned members are dropped.  Returns one NamedMatrix (sets x [size, rho, t,
    p.value, q.value]; [size, rho] with compute_p = False) ordered by `sort_by` (stable, NaN last; |rho| decreasing for
    "rho") when stat is a named vector; for a NamedMatrix, of one column or of many, a dict, column name -> NamedMatrix, in
    the columns' order.  p.value is the normal tail of the t-transform of rho, q.value Benjamini-Hochberg per list."""
    from .engine import rankcor_ties
    rankcor_ties(ties)   # (an unknown method is refused before anything else)
    if isinstance(stat, dict):
        stat = NamedMatrix(np.array(list(stat.values()), dtype=np.float64), list(stat.keys()), ["stat"])
        single = True
    else:
        single = not isinstance(stat, NamedMatrix) and np.ndim(stat) == 1
        try:
            import pandas as pd
            if isinstance(stat, pd.Series):
                stat, single = NamedMatrix(stat.to_numpy(dtype=np.float64), list(stat.index), ["stat"]), True
        except ImportError:  # pragma: no cover
            pass
    if isinstance(G, (GmtList, dict)) or (isinstance(G, tuple) and len(G) == 2):
        _message("[plaid.rankcor] converting gmt to sparse matrix...")
        G = gmt2mat(G)
    stat = as_named(stat)
    if sp.issparse(stat.values):
        raise ValueError("plaid.rankcor: stat must be dense")
    Xs, Gp, Gi, _, _, _, _, rn = _plaid_test_operands(stat, G, None, "one", "fisher")
    N = Xs.shape[0]
    sizes = np.diff(Gp)
    hi = N - 1 if maxSize is None else int(maxSize)
    keep = np.flatnonzero((sizes >= int(minSize)) & (sizes <= hi))
    Gi = np.concatenate([Gi[Gp[j]:Gp[j + 1]] for j in keep]).astype(np.int32) if len(keep) else np.zeros(0, np.int32)
    Gp = np.concatenate([[0], np.cumsum(sizes[keep])]).astype(np.int32)
    rn = [rn[j] for j in keep]
    ctx = ctx or default_context()
    out, _ = ctx.rankcor(Xs, Gp, Gi, use_rank=use_rank, ties=ties)
    cols = _RANKCOR_NAMES if compute_p else _RANKCOR_NAMES[:2]
    res = {}
    for l, nm in enumerate(stat.colnames):
        tab, names = out[:, :len(cols), l], list(rn)
        if sort_by in cols:
            key = tab[:, cols.index(sort_by)]
            o = np.argsort(-np.abs(key) if sort_by == "rho" else key, kind="stable")       # order(): NaN last
            tab, names = tab[o, :], [names[k] for k in o]
        res[nm] = NamedMatrix(tab, names, list(cols))
    return res[stat.colnames[0]] if single and len(res) == 1 else res


_LIMMA_NAMES = ["logFC", "AveExpr", "t", "P.Value", "adj.P.Val", "sigma2"]
_LIMMA_HYPER = ["df.residual", "df.prior", "s2.prior", "n.ok"]
_LIMMA_HYPER_NA = _LIMMA_HYPER + ["df.pooled"]
_LIMMA_SORT = {"none": None, "P.Value": (3, 1), "P": (3, 1), "p": (3, 1), "t": (2, -1), "logFC": (0, -1), "AveExpr": (1, -1)}


def _limma_table(tab, rn, sort_by):
    """rows x 6 of the library -> the NamedMatrix plaid.limma returns: topTable's order for `sort_by` -- "none" (the rows of
    S), "P.Value" / "P" / "p" (increasing), "t" and "logFC" (decreasing magnitude), "AveExpr" (decreasing); stable, NaN last"""
    if sort_by not in _LIMMA_SORT:
        raise ValueError(f"plaid.limma: sort_by must be one of {sorted(_LIMMA_SORT)}")
    rn = list(rn)
    if _LIMMA_SORT[sort_by] is not None:
        col, sign = _LIMMA_SORT[sort_by]
        key = tab[:, col] if sign > 0 else -np.abs(tab[:, col]) if col != 1 else -tab[:, col]
        o = np.argsort(key, kind="stable")
        tab, rn = tab[o, :], [rn[k] for k in o]
    return NamedMatrix(tab, rn, _LIMMA_NAMES + ["df.residual"][:tab.shape[1] - 6])


def _limma_weights(S, weights):
    """weights of plaid_limma as Context.limma takes them: a NamedMatrix or matrix in S's shape, or a vector over the samples"""
    if weights is None:
        return None
    w = np.asarray(weights.values if isinstance(weights, NamedMatrix) else weights, dtype=np.float64)
    if w.ndim == 2 and w.shape != S.values.shape:
        raise ValueError("plaid.limma: a matrix of weights has the shape of S")
    if w.ndim == 1 and w.shape[0] != S.values.shape[1]:
        raise ValueError("plaid.limma: a vector of weights has one entry per sample")
    if w.ndim not in (1, 2):
        raise ValueError("plaid.limma: weights are a matrix in S's shape or a vector over the samples")
    return w


def _limma_run(ctx, A, design, use, contrasts, na, max_na, weights=None):
    """(out rows x 6 or 7 x q x nfit, hyper, its names): under na = "fit" or with weights the rows' df.residual is the seventh
    column"""
    if na == "propagate" and weights is None:
        out, hyper = ctx.limma(A, design, use, contrasts)
        return out, hyper, _LIMMA_HYPER
    if weights is None:
        out, hyper, dfres = ctx.limma(A, design, use, contrasts, na=na, max_na=max_na)
    else:
        out, hyper, dfres = ctx.limma(A, design, use, contrasts, na=na, max_na=max_na, weights=weights)
    dfr = np.broadcast_to(dfres[:, None, None, :], (out.shape[0], 1, out.shape[2], out.shape[3]))
    dfr = np.where(np.isnan(out[:, 5:6, :, :]), np.nan, dfr)
    return np.concatenate([out, dfr], axis=1), hyper, _LIMMA_HYPER_NA


def plaid_limma(S, design, contrasts=None, use=None, sort_by="none", ctx: Context | None = None, na="propagate", max_na=0.2,
                weights=None):
    """plaid.limma(): limma's moderated t-test (lmFit + eBayes + topTable, as pinned in include/plaidhip.h) of every row of S
    -- a NamedMatrix of single-sample scores (sets x samples) or of expression (genes x samples) -- for one design (samples
    x coefficients; a NamedMatrix names the coefficients).  contrasts: coefficients x contrasts (a NamedMatrix names them),
    None: every coefficient.  use: one entry per sample, False / 0 / NaN leaves it out of the fit (a NaN or Inf it holds in
    S does not reach the fit).  Returns (tables, hyper): tables is a dict, contrast name -> NamedMatrix (rows x [logFC,
    AveExpr, t, P.Value, adj.P.Val, sigma2]) ordered by `sort_by`; hyper a dict of df.residual, df.prior, s2.prior and n.ok.
    The logFC and P.Value columns are what plaid_sig and plaid_gsea take.
    na: "propagate" (a NaN in a used sample makes the row NaN) or "fit": limma's own handling -- a row with at most the
    share max_na of NaN over all samples (gx.limma's max.na) is refitted on the samples it has, with its own df.residual
    and stdev.unscaled, and eBayes takes the unequal df; a row above max_na, or one that is not estimable on what it has,
    is NaN.  The tables then have a seventh column df.residual and hyper has df.pooled; at most 10 coefficients.
    weights: None, a matrix in S's shape (observation weights, limma's `weights`: voom's, or quality weights from upstream) or
    a vector over the samples (array weights).  The fit is then the weighted least squares of every row (plaidhip_limma_w): an
    observation with a NaN value or a weight that is zero, negative, NaN or infinite is missing, as in limma; the tables are
    those of na = "fit" (na = "propagate" then fits no row that holds a NaN); at most 10 coefficients.
    Not offered: trend, robust, the B- and F-statistics, a sparse S; weights in the set tests."""
    S = as_named(S)
    if S.is_sparse:
        raise ValueError("plaid.limma: S must be dense")
    Dn = design if isinstance(design, NamedMatrix) else None
    Dv = np.asarray(Dn.values if Dn is not None else design, dtype=np.float64)
    if Dv.ndim != 2:
        raise ValueError("plaid.limma: design must be samples x coefficients")
    coef = list(Dn.colnames) if Dn is not None else [f"coef{k + 1}" for k in range(Dv.shape[1])]
    if contrasts is None:
        Kv, names = None, coef
    else:
        Kn = contrasts if isinstance(contrasts, NamedMatrix) else None
        Kv = np.asarray(Kn.values if Kn is not None else contrasts, dtype=np.float64)
        Kv = Kv[:, None] if Kv.ndim == 1 else Kv
        names = list(Kn.colnames) if Kn is not None else [str(j + 1) for j in range(Kv.shape[1])]
    _limma_table(np.zeros((0, 6)), [], sort_by)   # (an unknown sort_by is refused before the device)
    wts = _limma_weights(S, weights)              # (and weights of another shape)
    ctx = ctx or default_context()
    out, hyper, hnames = _limma_run(ctx, S.values, Dv, use, Kv, na, max_na, wts)
    tables = {nm: _limma_table(out[:, :, j, 0], S.rownames, sort_by) for j, nm in enumerate(names)}
    return tables, dict(zip(hnames, (float(x) for x in hyper[0])))


def plaid_voom(counts, design, lib_size=None, span=0.5, ctx: Context | None = None):
    """plaid.voom(): limma's voom with normalize.method = "none" (as pinned in include/plaidhip.h: plaidhip_voom) of a counts
    matrix (genes x samples, finite and >= 0) for one design (samples x coefficients).  lib_size: one entry per sample, None: the
    column sums.  span: the lowess span of the mean-variance trend.  Returns a dict: E (NamedMatrix of log2-CPM), weights
    (NamedMatrix of precision weights), lib.size, offset (log2(lib.size + 1) - log2(1e6)) and the trend's knots (knots.x,
    knots.y).  plaid_limma(E, design, weights=weights) is limma's lmFit + eBayes on that EList.
    Not offered: other normalize.method, voomWithQualityWeights, arrayWeights, duplicateCorrelation, sparse counts."""
    S = as_named(counts)
    if S.is_sparse:
        raise ValueError("plaid.voom: counts must be dense")
    Dv = np.asarray(design.values if isinstance(design, NamedMatrix) else design, dtype=np.float64)
    if Dv.ndim != 2 or Dv.shape[0] != S.values.shape[1]:
        raise ValueError("plaid.voom: design must be samples x coefficients, one row per column of counts")
    if not (0.0 < float(span) <= 1.0):
        raise ValueError("plaid.voom: span must lie in (0, 1]")
    ctx = ctx or default_context()
    r = ctx.voom(S.values, Dv, lib_size, span)
    return {"E": NamedMatrix(r["E"], S.rownames, S.colnames), "weights": NamedMatrix(r["weights"], S.rownames, S.colnames),
            "lib.size": r["lib_size"], "offset": r["offset"], "knots.x": r["knots_x"], "knots.y": r["knots_y"]}


def plaid_limma_contrasts(S, Y, B=None, sort_by="none", ctx: Context | None = None, na="propagate", max_na=0.2, weights=None):
    """plaid.limma.contrasts(): the reference's gx.limma(S, y, B, method = 1) for every column of the contrast matrix Y
    (samples x contrasts; 0, 1, and NaN or -1 for a sample that takes no part) in one call: contrast j fits the design
    [1, Y[, j], B] on the samples with a label and tests the coefficient of Y[, j].  B: batch covariates, samples x
    covariates, or None.  S is uploaded once and read ceil(C (p + 1) / 8) times for the effects, p = 2 + ncol(B).  Y: a
    NamedMatrix (its column names name the contrasts) or an array (contrasts "1", "2", ...).  Returns (tables, hyper):
    contrast name -> the NamedMatrix plaid_limma returns, and contrast name -> its hyper-parameters.  na, max_na: as
    plaid_limma; with na = "fit" and max_na = 0.2 this is gx.limma(S, y, B, max.na = 0.2) on a matrix with missing values.
    weights: as plaid_limma, shared by the contrasts."""
    from .engine import contrast_labels
    S = as_named(S)
    if S.is_sparse:
        raise ValueError("plaid.limma: S must be dense")
    n = S.shape[1]
    Yn = Y if isinstance(Y, NamedMatrix) else None
    lab = contrast_labels(Yn.values if Yn is not None else Y, n)
    if not np.all(np.isin(lab, (0, 1, -1))):
        raise ValueError("elements of Y must be 0, 1 or NA")
    ncon = lab.shape[1]
    names = list(Yn.colnames) if Yn is not None and Yn.colnames is not None else [str(j + 1) for j in range(ncon)]
    Bv = np.zeros((n, 0)) if B is None else np.asarray(B.values if isinstance(B, NamedMatrix) else B, dtype=np.float64)
    Bv = Bv[:, None] if Bv.ndim == 1 else Bv
    if Bv.ndim != 2 or Bv.shape[0] != n:
        raise ValueError("B must have one row per column of S")
    p = 2 + Bv.shape[1]
    D = np.empty((n, p, ncon), order="F")
    D[:, 0, :] = 1.0
    D[:, 1, :] = np.where(lab == 1, 1.0, 0.0)
    D[:, 2:, :] = Bv[:, :, None]
    K = np.zeros((p, 1))
    K[1, 0] = 1.0
    _limma_table(np.zeros((0, 6)), [], sort_by)
    wts = _limma_weights(S, weights)
    ctx = ctx or default_context()
    out, hyper, hnames = _limma_run(ctx, S.values, D, lab != -1, K, na, max_na, wts)
    tables = {nm: _limma_table(out[:, :, 0, j], S.rownames, sort_by) for j, nm in enumerate(names)}
    return tables, {nm: dict(zip(hnames, (float(x) for x in hyper[j]))) for j, nm in enumerate(names)}


_CAMERA_NAMES = ["NGenes", "Correlation", "VIF", "t", "Direction", "PValue", "FDR"]
_CAMERA_SORT = {"none": None, "PValue": 5, "P": 5, "p": 5, "FDR": 6, "t": 3, "Correlation": 1, "VIF": 2, "NGenes": 0}


def _camera_table(tab, rn, sort_by):
    """sets x 8 of the library -> the NamedMatrix plaid.camera returns: Direction is +1 (Up) where Up < Down, else -1 (Down),
    NaN on a NaN row; ordered by `sort_by` -- "none", "PValue" / "P" / "p" and "FDR" (increasing), "t", "Correlation", "VIF"
    (decreasing magnitude), "NGenes" (decreasing); stable, NaN last"""
    if sort_by not in _CAMERA_SORT:
        raise ValueError(f"plaid.camera: sort_by must be one of {sorted(_CAMERA_SORT)}")
    down, up = tab[:, 4], tab[:, 5]
    direction = np.where(np.isnan(up) | np.isnan(down), np.nan, np.where(up < down, 1.0, -1.0))
    tab = np.column_stack([tab[:, 0:4], direction, tab[:, 6:8]])
    rn = list(rn)
    col = _CAMERA_SORT[sort_by]
    if col is not None:
        key = tab[:, col] if col in (5, 6) else -tab[:, col] if col == 0 else -np.abs(tab[:, col])
        o = np.argsort(key, kind="stable")
        tab, rn = tab[o, :], [rn[k] for k in o]
    return NamedMatrix(tab, rn, _CAMERA_NAMES)


def _camera_sets(who, X, G, minSize, maxSize):
    """X (genes x samples, a NamedMatrix) and G (a gmt or a membership matrix): every row of X stays -- camera's universe is
    all the genes, also those in no set -- and the members of G are mapped to the rows of X by name (a name X does not have
    is dropped; the first of a repeated name counts).  Sets outside minSize .. maxSize (default: the genes - 1) mapped members
    are dropped: (Xs, Gp, Gi, names)"""
    if isinstance(G, (GmtList, dict)) or (isinstance(G, tuple) and len(G) == 2):
        _message(f"[{who}] converting gmt to sparse matrix...")
        G = gmt2mat(G)
    X, G = as_named(X), as_named(G)
    if X.is_sparse:
        raise ValueError(f"{who}: X must be dense")
    posx = _first_pos(X.rownames)
    seen, grow, xrow = set(), [], []
    for k, nm in enumerate(G.rownames):
        if nm in seen:
            continue
        seen.add(nm)
        r = posx.get(nm)
        if r is not None:
            grow.append(k)
            xrow.append(r)
    Gs = sp.csc_matrix(G.values)[grow, :].tocsc()
    xrow = np.asarray(xrow, dtype=np.int32)
    sets = [np.sort(xrow[Gs.indices[Gs.indptr[j]:Gs.indptr[j + 1]][Gs.data[Gs.indptr[j]:Gs.indptr[j + 1]] != 0]])
            for j in range(Gs.shape[1])]
    hi = X.shape[0] - 1 if maxSize is None else int(maxSize)
    keep = [j for j, s_ in enumerate(sets) if int(minSize) <= len(s_) <= hi]
    Gi = np.concatenate([sets[j] for j in keep]).astype(np.int32) if keep else np.zeros(0, np.int32)
    Gp = np.concatenate([[0], np.cumsum([len(sets[j]) for j in keep])]).astype(np.int32)
    return np.asfortranarray(np.asarray(X.values), dtype=np.float64), Gp, Gi, [G.colnames[j] for j in keep]


def plaid_camera(X, design, G, contrasts=None, use=None, inter_gene_cor=0.01, allow_neg_cor=False, minSize=1, maxSize=None,
                 sort_by="PValue", ctx: Context | None = None):
    """plaid.camera(): limma's competitive gene-set test camera (Wu & Smyth 2012, as pinned in include/plaidhip.h) of every set
    of G (a gmt or a membership matrix) on the expression X (a genes x samples NamedMatrix) for one design (samples x
    coefficients; a NamedMatrix names the coefficients).  contrasts, use: as plaid_limma.  The gene statistic is
    plaid_limma's moderated t; a set's two-sample t against the other genes is corrected by the variance inflation factor
    1 + (m - 1) rho.  inter_gene_cor: the fixed rho (limma's default 0.01), or None to estimate every set's VIF from the
    residuals of its genes (allow_neg_cor = False then uses max(VIF, 1) in the test; the reported VIF and Correlation stay
    as estimated).  The universe is every row of X, also the genes in no set; the members of G are found in X by name.  A
    gene with a NaN or Inf in a used sample leaves the universe.  Sets with fewer than minSize or more than maxSize
    (default: the genes - 1) members in X are dropped.  Returns (tables, hyper): tables is a dict, contrast name -> NamedMatrix (sets x [NGenes, Correlation, VIF, t,
    Direction (+1 Up, -1 Down), PValue, FDR]) ordered by `sort_by` (default "PValue"; stable, NaN last); hyper a dict of
    plaid_limma's four values, n.genes and df.camera.
    Not offered: use.ranks, trend.var, weights, a sparse X, na = "fit", fry / roast."""
    Xs, Gp, Gi, rn = _camera_sets("plaid.camera", X, G, minSize, maxSize)
    Dn = design if isinstance(design, NamedMatrix) else None
    Dv = np.asarray(Dn.values if Dn is not None else design, dtype=np.float64)
    if Dv.ndim != 2:
        raise ValueError("plaid.camera: design must be samples x coefficients")
    coef = list(Dn.colnames) if Dn is not None else [f"coef{k + 1}" for k in range(Dv.shape[1])]
    if contrasts is None:
        Kv, names = None, coef
    else:
        Kn = contrasts if isinstance(contrasts, NamedMatrix) else None
        Kv = np.asarray(Kn.values if Kn is not None else contrasts, dtype=np.float64)
        Kv = Kv[:, None] if Kv.ndim == 1 else Kv
        names = list(Kn.colnames) if Kn is not None else [str(j + 1) for j in range(Kv.shape[1])]
    _camera_table(np.zeros((0, 8)), [], sort_by)   # (an unknown sort_by and a correlation outside (-1, 1): before the device)
    from .engine import CAMERA_HYPER, check_camera_cor
    check_camera_cor(inter_gene_cor)
    ctx = ctx or default_context()
    out, hyper = ctx.camera(Xs, Dv, Gp, Gi, use, Kv, inter_gene_cor, allow_neg_cor)
    tables = {nm: _camera_table(out[:, :, j, 0], rn, sort_by) for j, nm in enumerate(names)}
    return tables, dict(zip(CAMERA_HYPER, (float(x) for x in hyper[0])))


def plaid_camera_contrasts(X, Y, G, B=None, inter_gene_cor=0.01, allow_neg_cor=False, minSize=1, maxSize=None,
                           sort_by="PValue", ctx: Context | None = None):
    """plaid.camera.contrasts(): plaid_camera for every column of the contrast matrix Y (samples x contrasts; 0, 1, and NaN or
    -1 for a sample that takes no part) in one call, with the designs of plaid_limma_contrasts: contrast j fits [1, Y[, j], B]
    on the samples with a label and tests the sets on the moderated t of the coefficient of Y[, j].  X is uploaded once.
    Returns (tables, hyper): contrast name -> the NamedMatrix plaid_camera returns, and contrast name -> its
    hyper-parameters.  Contrast j has the bits of plaid_camera on that contrast's design and samples."""
    from .engine import CAMERA_HYPER, check_camera_cor, contrast_labels
    check_camera_cor(inter_gene_cor)
    Xs, Gp, Gi, rn = _camera_sets("plaid.camera", X, G, minSize, maxSize)
    n = Xs.shape[1]
    Yn = Y if isinstance(Y, NamedMatrix) else None
    lab = contrast_labels(Yn.values if Yn is not None else Y, n)
    if not np.all(np.isin(lab, (0, 1, -1))):
        raise ValueError("elements of Y must be 0, 1 or NA")
    ncon = lab.shape[1]
    names = list(Yn.colnames) if Yn is not None and Yn.colnames is not None else [str(j + 1) for j in range(ncon)]
    Bv = np.zeros((n, 0)) if B is None else np.asarray(B.values if isinstance(B, NamedMatrix) else B, dtype=np.float64)
    Bv = Bv[:, None] if Bv.ndim == 1 else Bv
    if Bv.ndim != 2 or Bv.shape[0] != n:
        raise ValueError("B must have one row per column of X")
    p = 2 + Bv.shape[1]
    D = np.empty((n, p, ncon), order="F")
    D[:, 0, :] = 1.0
    D[:, 1, :] = np.where(lab == 1, 1.0, 0.0)
    D[:, 2:, :] = Bv[:, :, None]
    K = np.zeros((p, 1))
    K[1, 0] = 1.0
    _camera_table(np.zeros((0, 8)), [], sort_by)
    ctx = ctx or default_context()
    out, hyper = ctx.camera(Xs, D, Gp, Gi, lab != -1, K, inter_gene_cor, allow_neg_cor)
    tables = {nm: _camera_table(out[:, :, 0, j], rn, sort_by) for j, nm in enumerate(names)}
    return tables, {nm: dict(zip(CAMERA_HYPER, (float(x) for x in hyper[j]))) for j, nm in enumerate(names)}


_FRY_NAMES = ["NGenes", "Direction", "t", "PValue", "FDR", "PValue.Mixed", "FDR.Mixed"]
_FRY_SORT = {"none": None, "directional": 3, "mixed": 5}


def _fry_table(tab, rn, sort_by):
    """sets x 7 of the library -> the NamedMatrix plaid.fry returns (Direction +1 Up, -1 Down), ordered by `sort_by`:
    "directional" (PValue increasing), "mixed" (PValue.Mixed increasing) or "none"; stable, NaN last"""
    if sort_by not in _FRY_SORT:
        raise ValueError(f"plaid.fry: sort_by must be one of {sorted(_FRY_SORT)}")
    rn = list(rn)
    col = _FRY_SORT[sort_by]
    if col is not None:
        o = np.argsort(tab[:, col], kind="stable")
        tab, rn = tab[o, :], [rn[k] for k in o]
    return NamedMatrix(np.ascontiguousarray(tab), rn, _FRY_NAMES)


def plaid_fry(X, design, G, contrasts=None, use=None, standardize="posterior.sd", minSize=1, maxSize=None,
              sort_by="directional", ctx: Context | None = None):
    """plaid.fry(): limma's self-contained rotation gene-set test in closed form (fry: roast with infinitely many rotations,
    as pinned in include/plaidhip.h) of every set of G on the expression X for one design; the operands are plaid_camera's.
    camera asks whether a set moves more than the other genes, fry whether the set is differential at all; it draws no
    random number.  standardize: "posterior.sd" (the default: the effects are plaid_limma's moderated t), "residual.sd" or
    "none".  A gene with a NaN or Inf in a used sample, or with a divisor that is 0, leaves the universe.  The directional
    test is complete for any number of samples; the mixed test (a set whose genes move in both directions) is offered for
    fits with df.residual + 1 <= 128 effects, and NaN above that (hyper["mixed"] = 0).  Returns (tables, hyper): contrast
    name -> NamedMatrix (sets x [NGenes, Direction (+1 Up, -1 Down), t, PValue, FDR, PValue.Mixed, FDR.Mixed]) ordered by
    `sort_by` ("directional", "mixed" or "none"; stable, NaN last), and plaid_limma's four values, n.genes, n.effects
    (df.residual + 1) and mixed.
    Not offered: roast / mroast, gene or array weights, trend.var, robust, a sparse X, na = "fit", standardize = "p2"."""
    from .engine import FRY_HYPER, check_fry_standardize
    check_fry_standardize(standardize)
    _fry_table(np.zeros((0, 7)), [], sort_by)   # (an unknown sort_by: before the device)
    Xs, Gp, Gi, rn = _camera_sets("plaid.fry", X, G, minSize, maxSize)
    Dn = design if isinstance(design, NamedMatrix) else None
    Dv = np.asarray(Dn.values if Dn is not None else design, dtype=np.float64)
    if Dv.ndim != 2:
        raise ValueError("plaid.fry: design must be samples x coefficients")
    coef = list(Dn.colnames) if Dn is not None else [f"coef{k + 1}" for k in range(Dv.shape[1])]
    if contrasts is None:
        Kv, names = None, coef
    else:
        Kn = contrasts if isinstance(contrasts, NamedMatrix) else None
        Kv = np.asarray(Kn.values if Kn is not None else contrasts, dtype=np.float64)
        Kv = Kv[:, None] if Kv.ndim == 1 else Kv
        names = list(Kn.colnames) if Kn is not None else [str(j + 1) for j in range(Kv.shape[1])]
    ctx = ctx or default_context()
    out, hyper = ctx.fry(Xs, Dv, Gp, Gi, use, Kv, standardize)
    tables = {nm: _fry_table(out[:, :, j, 0], rn, sort_by) for j, nm in enumerate(names)}
    return tables, dict(zip(FRY_HYPER, (float(x) for x in hyper[0])))


def plaid_fry_contrasts(X, Y, G, B=None, standardize="posterior.sd", minSize=1, maxSize=None, sort_by="directional",
                        ctx: Context | None = None):
    """plaid.fry.contrasts(): plaid_fry for every column of the contrast matrix Y in one call, with the designs of
    plaid_limma_contrasts: contrast j fits [1, Y[, j], B] on the samples with a label and tests the sets on the coefficient
    of Y[, j].  X is uploaded once.  Returns (tables, hyper) keyed by contrast name; contrast j has the bits of plaid_fry on
    that contrast's design and samples."""
    from .engine import FRY_HYPER, check_fry_standardize, contrast_labels
    check_fry_standardize(standardize)
    _fry_table(np.zeros((0, 7)), [], sort_by)
    Xs, Gp, Gi, rn = _camera_sets("plaid.fry", X, G, minSize, maxSize)
    n = Xs.shape[1]
    Yn = Y if isinstance(Y, NamedMatrix) else None
    lab = contrast_labels(Yn.values if Yn is not None else Y, n)
    if not np.all(np.isin(lab, (0, 1, -1))):
        raise ValueError("elements of Y must be 0, 1 or NA")
    ncon = lab.shape[1]
    names = list(Yn.colnames) if Yn is not None and Yn.colnames is not None else [str(j + 1) for j in range(ncon)]
    Bv = np.zeros((n, 0)) if B is None else np.asarray(B.values if isinstance(B, NamedMatrix) else B, dtype=np.float64)
    Bv = Bv[:, None] if Bv.ndim == 1 else Bv
    if Bv.ndim != 2 or Bv.shape[0] != n:
        raise ValueError("B must have one row per column of X")
    p = 2 + Bv.shape[1]
    D = np.empty((n, p, ncon), order="F")
    D[:, 0, :] = 1.0
    D[:, 1, :] = np.where(lab == 1, 1.0, 0.0)
    D[:, 2:, :] = Bv[:, :, None]
    K = np.zeros((p, 1))
    K[1, 0] = 1.0
    ctx = ctx or default_context()
    out, hyper = ctx.fry(Xs, D, Gp, Gi, lab != -1, K, standardize)
    tables = {nm: _fry_table(out[:, :, 0, j], rn, sort_by) for j, nm in enumerate(names)}
    return tables, {nm: dict(zip(FRY_HYPER, (float(x) for x in hyper[j]))) for j, nm in enumerate(names)}


_ROAST_NAMES = ["NGenes", "PropDown", "PropUp", "Direction", "PValue", "FDR", "PValue.Mixed", "FDR.Mixed"]
_ROAST_SORT = {"none": None, "directional": 4, "mixed": 6}


def _roast_table(tab, rn, sort_by):
    """sets x 8 of the library -> the NamedMatrix plaid.roast returns (Direction +1 Up, -1 Down), ordered by `sort_by`:
    "directional" (PValue increasing), "mixed" (PValue.Mixed increasing) or "none"; stable, NaN last"""
    rn = list(rn)
    col = _ROAST_SORT[sort_by]
    if col is not None:
        o = np.argsort(tab[:, col], kind="stable")
        tab, rn = tab[o, :], [rn[k] for k in o]
    return NamedMatrix(np.ascontiguousarray(tab), rn, _ROAST_NAMES)


def plaid_roast(X, design, G, contrasts=None, use=None, set_statistic="mean50", nrot=1999, seed=1, zscore="hill", midp=True,
                rotations=None, minSize=1, maxSize=None, sort_by="directional", ctx: Context | None = None):
    """plaid.roast(): limma's rotation gene-set test with sampled rotations (roast / mroast as pinned in
    include/plaidhip.h) of every set of G on the expression X for one design; the operands are plaid_fry's.  What it adds
    to plaid_fry: a mixed test for any number of samples, and the set statistics "mean50" (the default), "floormean" and
    "msq" beside "mean".  The rotations are drawn in sample space from `seed` (Philox4x32-10) and shared by every set and
    contrast -- or given: rotations, (samples + 1) x nrot with row 0 = r0.  zscore: "hill" (the default) or "none".  p =
    (b + 1) / (nrot + 1); midp takes the FDR on p - 0.5 / (nrot + 1).  A gene with a NaN or Inf in a used sample leaves the
    universe; under "mean50" a set with more than 16,384 members there has NaN p-values (hyper["mean50.capped"] = 1).
    Returns (tables, hyper): contrast name -> NamedMatrix (sets x [NGenes, PropDown, PropUp, Direction (+1 Up, -1 Down),
    PValue, FDR, PValue.Mixed, FDR.Mixed]) ordered by `sort_by` ("directional", "mixed" or "none"; stable, NaN last), and
    plaid_limma's four values, n.genes, nrot and mean50.capped.
    Not offered: per-set rotations, gene or array weights, trend.var, robust, a sparse X, na = "fit"; romer is plaid_romer,
    below."""
    from .engine import ROAST_HYPER, check_roast_options
    check_roast_options(set_statistic, zscore)
    if sort_by not in _ROAST_SORT:   # (before the device)
        raise ValueError(f"plaid.roast: sort_by must be one of {sorted(_ROAST_SORT)}")
    Xs, Gp, Gi, rn = _camera_sets("plaid.roast", X, G, minSize, maxSize)
    Dn = design if isinstance(design, NamedMatrix) else None
    Dv = np.asarray(Dn.values if Dn is not None else design, dtype=np.float64)
    if Dv.ndim != 2:
        raise ValueError("plaid.roast: design must be samples x coefficients")
    coef = list(Dn.colnames) if Dn is not None else [f"coef{k + 1}" for k in range(Dv.shape[1])]
    if contrasts is None:
        Kv, names = None, coef
    else:
        Kn = contrasts if isinstance(contrasts, NamedMatrix) else None
        Kv = np.asarray(Kn.values if Kn is not None else contrasts, dtype=np.float64)
        Kv = Kv[:, None] if Kv.ndim == 1 else Kv
        names = list(Kn.colnames) if Kn is not None else [str(j + 1) for j in range(Kv.shape[1])]
    ctx = ctx or default_context()
    out, hyper = ctx.roast(Xs, Dv, Gp, Gi, use, Kv, set_statistic, nrot, seed, zscore, midp, rotations)
    tables = {nm: _roast_table(out[:, :, j, 0], rn, sort_by) for j, nm in enumerate(names)}
    return tables, dict(zip(ROAST_HYPER, (float(x) for x in hyper[0])))


def plaid_roast_contrasts(X, Y, G, B=None, set_statistic="mean50", nrot=1999, seed=1, zscore="hill", midp=True, rotations=None,
                          minSize=1, maxSize=None, sort_by="directional", ctx: Context | None = None):
    """plaid.roast.contrasts(): plaid_roast for every column of the contrast matrix Y in one call, with the designs of
    plaid_limma_contrasts: contrast j fits [1, Y[, j], B] on the samples with a label and tests the sets on the coefficient
    of Y[, j].  X is uploaded once.  Contrast j is fit number j: its generated rotations are those of (seed, j), so its
    table has the bits of plaid_roast on that contrast's design and samples only for j = 0 -- or for any j where
    `rotations` ((samples + 1) x nrot x contrasts) are given.  Returns (tables, hyper) keyed by contrast name."""
    from .engine import ROAST_HYPER, check_roast_options, contrast_labels
    check_roast_options(set_statistic, zscore)
    if sort_by not in _ROAST_SORT:
        raise ValueError(f"plaid.roast: sort_by must be one of {sorted(_ROAST_SORT)}")
    Xs, Gp, Gi, rn = _camera_sets("plaid.roast", X, G, minSize, maxSize)
    n = Xs.shape[1]
    Yn = Y if isinstance(Y, NamedMatrix) else None
    lab = contrast_labels(Yn.values if Yn is not None else Y, n)
    if not np.all(np.isin(lab, (0, 1, -1))):
        raise ValueError("elements of Y must be 0, 1 or NA")
    ncon = lab.shape[1]
    names = list(Yn.colnames) if Yn is not None and Yn.colnames is not None else [str(j + 1) for j in range(ncon)]
    Bv = np.zeros((n, 0)) if B is None else np.asarray(B.values if isinstance(B, NamedMatrix) else B, dtype=np.float64)
    Bv = Bv[:, None] if Bv.ndim == 1 else Bv
    if Bv.ndim != 2 or Bv.shape[0] != n:
        raise ValueError("B must have one row per column of X")
    p = 2 + Bv.shape[1]
    D = np.empty((n, p, ncon), order="F")
    D[:, 0, :] = 1.0
    D[:, 1, :] = np.where(lab == 1, 1.0, 0.0)
    D[:, 2:, :] = Bv[:, :, None]
    K = np.zeros((p, 1))
    K[1, 0] = 1.0
    ctx = ctx or default_context()
    out, hyper = ctx.roast(Xs, D, Gp, Gi, lab != -1, K, set_statistic, nrot, seed, zscore, midp, rotations)
    tables = {nm: _roast_table(out[:, :, 0, j], rn, sort_by) for j, nm in enumerate(names)}
    return tables, {nm: dict(zip(ROAST_HYPER, (float(x) for x in hyper[j]))) for j, nm in enumerate(names)}


_ROMER_NAMES = ["NGenes", "Up", "Down", "Mixed", "FDR.Up", "FDR.Down", "FDR.Mixed"]
_ROMER_SORT = {"none": None, "up": 1, "down": 2, "mixed": 3}


def _romer_table(tab, rn, sort_by):
    """sets x 7 of the library -> the NamedMatrix plaid.romer returns, ordered by `sort_by`: "up", "down", "mixed" (that
    p-value increasing) or "none"; stable, NaN last"""
    rn = list(rn)
    col = _ROMER_SORT[sort_by]
    if col is not None:
        o = np.argsort(tab[:, col], kind="stable")
        tab, rn = tab[o, :], [rn[k] for k in o]
    return NamedMatrix(np.ascontiguousarray(tab), rn, _ROMER_NAMES)


def _romer_hyper(h, names):
    from .engine import ROMER_HYPER
    d = dict(zip(ROMER_HYPER, (float(x) for x in h[:8])))
    d["proportion"] = {nm: float(h[8 + j]) for j, nm in enumerate(names)}
    return d


def plaid_romer(X, design, G, contrasts=None, use=None, set_statistic="mean", nrot=9999, seed=1, shrink_resid=True,
                rotations=None, minSize=1, maxSize=None, sort_by="none", ctx: Context | None = None):
    """plaid.romer(): limma's rotation GSEA (romer as pinned in include/plaidhip.h) of every set of G on the expression X for
    one design; the operands are plaid_roast's.  It is the competitive test with a rotation null: under every rotation the
    genes' moderated t are ranked among all genes and a set takes the sum of its members' ranks, so the null keeps the
    gene-gene correlation.  set_statistic: "mean" (the default), "floormean" or "mean50".  shrink_resid (limma's default)
    shrinks the observed effects by the empirical-Bayes posterior before rotating.  The rotations are drawn in sample space
    from `seed` (plaid_roast's, shared by every set and contrast) -- or given: rotations, (samples + 1) x nrot with row 0 =
    r0.  p = (b + 1) / (nrot + 1) from exact integer statistics.  Under "mean50" a set with more than 16,384 members in the
    universe has NaN p-values (hyper["mean50.capped"] = 1).
    Returns (tables, hyper): contrast name -> NamedMatrix (sets x [NGenes, Up, Down, Mixed, FDR.Up, FDR.Down, FDR.Mixed])
    ordered by `sort_by` ("up", "down", "mixed" or "none"), and plaid_limma's four values, n.genes, nrot, mean50.capped,
    nan.t and the proportion of non-null genes of every contrast (0 where not shrunk).
    Not offered: array.weights, block / correlation, a sparse X, na = "fit", gene weights, trend, robust."""
    from .engine import check_romer_options
    check_romer_options(set_statistic)
    if sort_by not in _ROMER_SORT:   # (before the device)
        raise ValueError(f"plaid.romer: sort_by must be one of {sorted(_ROMER_SORT)}")
    Xs, Gp, Gi, rn = _camera_sets("plaid.romer", X, G, minSize, maxSize)
    Dn = design if isinstance(design, NamedMatrix) else None
    Dv = np.asarray(Dn.values if Dn is not None else design, dtype=np.float64)
    if Dv.ndim != 2:
        raise ValueError("plaid.romer: design must be samples x coefficients")
    coef = list(Dn.colnames) if Dn is not None else [f"coef{k + 1}" for k in range(Dv.shape[1])]
    if contrasts is None:
        Kv, names = None, coef
    else:
        Kn = contrasts if isinstance(contrasts, NamedMatrix) else None
        Kv = np.asarray(Kn.values if Kn is not None else contrasts, dtype=np.float64)
        Kv = Kv[:, None] if Kv.ndim == 1 else Kv
        names = list(Kn.colnames) if Kn is not None else [str(j + 1) for j in range(Kv.shape[1])]
    ctx = ctx or default_context()
    out, hyper = ctx.romer(Xs, Dv, Gp, Gi, use, Kv, set_statistic, nrot, seed, shrink_resid, None, rotations)
    tables = {nm: _romer_table(out[:, :, j, 0], rn, sort_by) for j, nm in enumerate(names)}
    return tables, _romer_hyper(hyper[0], names)


def plaid_romer_contrasts(X, Y, G, B=None, set_statistic="mean", nrot=9999, seed=1, shrink_resid=True, rotations=None,
                          minSize=1, maxSize=None, sort_by="none", ctx: Context | None = None):
    """plaid.romer.contrasts(): plaid_romer for every column of the contrast matrix Y in one call, with the designs of
    plaid_limma_contrasts: contrast j fits [1, Y[, j], B] on the samples with a label and tests the sets on the coefficient
    of Y[, j].  X is uploaded once.  Contrast j is fit number j: its generated rotations are those of (seed, j), so its
    table has the bits of plaid_romer on that contrast's design and samples only for j = 0 -- or for any j where
    `rotations` ((samples + 1) x nrot x contrasts) are given.  Returns (tables, hyper) keyed by contrast name."""
    from .engine import check_romer_options, contrast_labels
    check_romer_options(set_statistic)
    if sort_by not in _ROMER_SORT:
        raise ValueError(f"plaid.romer: sort_by must be one of {sorted(_ROMER_SORT)}")
    Xs, Gp, Gi, rn = _camera_sets("plaid.romer", X, G, minSize, maxSize)
    n = Xs.shape[1]
    Yn = Y if isinstance(Y, NamedMatrix) else None
    lab = contrast_labels(Yn.values if Yn is not None else Y, n)
    if not np.all(np.isin(lab, (0, 1, -1))):
        raise ValueError("elements of Y must be 0, 1 or NA")
    ncon = lab.shape[1]
    names = list(Yn.colnames) if Yn is not None and Yn.colnames is not None else [str(j + 1) for j in range(ncon)]
    Bv = np.zeros((n, 0)) if B is None else np.asarray(B.values if isinstance(B, NamedMatrix) else B, dtype=np.float64)
    Bv = Bv[:, None] if Bv.ndim == 1 else Bv
    if Bv.ndim != 2 or Bv.shape[0] != n:
        raise ValueError("B must have one row per column of X")
    p = 2 + Bv.shape[1]
    D = np.empty((n, p, ncon), order="F")
    D[:, 0, :] = 1.0
    D[:, 1, :] = np.where(lab == 1, 1.0, 0.0)
    D[:, 2:, :] = Bv[:, :, None]
    K = np.zeros((p, 1))
    K[1, 0] = 1.0
    ctx = ctx or default_context()
    out, hyper = ctx.romer(Xs, D, Gp, Gi, lab != -1, K, set_statistic, nrot, seed, shrink_resid, None, rotations)
    tables = {nm: _romer_table(out[:, :, 0, j], rn, sort_by) for j, nm in enumerate(names)}
    return tables, {nm: _romer_hyper(hyper[j], [nm]) for j, nm in enumerate(names)}


def plaid_intergenecor(X, design, G, use=None, minSize=1, maxSize=None, ctx: Context | None = None):
    """plaid.intergenecor(): limma's interGeneCorrelation(X[set, ], design) for every set of G at once -- the variance
    inflation factor of the set's mean, estimated from the residuals of its genes, and the mean pairwise correlation
    (VIF - 1) / (m - 1) it stands for.  Returns a NamedMatrix, sets x [NGenes, Correlation, VIF], in G's order."""
    Xs, Gp, Gi, rn = _camera_sets("plaid.intergenecor", X, G, minSize, maxSize)
    Dv = np.asarray(design.values if isinstance(design, NamedMatrix) else design, dtype=np.float64)
    if Dv.ndim != 2:
        raise ValueError("plaid.intergenecor: design must be samples x coefficients")
    K = np.zeros((Dv.shape[1], 1))
    K[0, 0] = 1.0   # (any contrast: the VIF does not depend on it)
    ctx = ctx or default_context()
    out, _ = ctx.camera(Xs, Dv, Gp, Gi, use, K, None, True)
    return NamedMatrix(np.ascontiguousarray(out[:, 0:3, 0, 0]), rn, _CAMERA_NAMES[:3])
