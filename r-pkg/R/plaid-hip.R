## R-side of the drop-in: the reference's signatures (R/plaid.R:60, :213, :244, :554, :589,
## :631 of bigomics/plaid) with bodies that hand the arithmetic to libplaidhip.so through
## .Call().  Gene-name alignment and dimnames stay in R; nothing numeric is computed here.
## A maintainer of the reference would add `useDynLib(plaidhip, .registration = TRUE)` to
## NAMESPACE and replace the bodies of the functions below (see INTEGRATION.md).

## Session options (set with options(); read on every call):
##   plaidhip.device     integer, the GPU ordinal the session context lives on (default 0; read when the
##                       context is first created)
##   plaidhip.devices    integer vector of GPU ordinals: with more than one, plaid() / replaid.sing() /
##                       replaid.ssgsea() / replaid.ucell() / replaid.aucell() / replaid.scse() / replaid.gsva() /
##                       plaid.test() shard the sample columns over them (a host thread per device inside the library,
##                       no process per GPU); replaid.gsva(rowtf = "ecdf") ranks all samples of a gene together and
##                       stays on the session device.  One ordinal: that GPU is the session device; default: the session device
##                       alone.  plaidhip.precision applies to every device of the list.
##   plaidhip.precision  "f64" (default: scores equal to the last bits) or "mixed" (dense crossprod stages the
##                       sample columns as fp32, sums fp64; ~1e-7 relative, inside the 1e-5 bar; ~1.5x faster)
## a single ordinal in plaidhip.devices IS the session device (it used to be ignored in favour of plaidhip.device)
.device <- function() {
  d <- getOption("plaidhip.devices", NULL)
  if (length(d) == 1L) return(as.integer(d))
  as.integer(getOption("plaidhip.device", 0L))
}
.devices <- function() as.integer(getOption("plaidhip.devices", .device()))
.session <- function() {
  prec <- match(getOption("plaidhip.precision", "f64"), c("f64", "mixed"))
  if (is.na(prec)) stop("options(plaidhip.precision) must be \"f64\" or \"mixed\"")
  .Call("R_plaidhip_session", .device(), prec - 1L, PACKAGE = "plaidhip")
  invisible(NULL)
}

.stat_code <- function(stats) match(stats[1], c("mean", "sum")) - 1L
## ties.method is passed through like the reference does (R/plaid.R:614-617, 639-642).  `allowed`: what the function
## behind the branch takes (match.arg there): matrixStats::colRanks all seven, base::rank no "dense",
## sparseMatrixStats::colRanks max / average / min.  "random" is refused by the library (not a function of the input).
.ties_all <- c("average", "min", "max", "first", "last", "dense", "random")
.ties_code <- function(ties.method, allowed = .ties_all) {
  ties.method <- match.arg(ties.method, allowed)
  match(ties.method, .ties_all) - 1L
}

## intersect + binarise (reference R/plaid.R:65-73) WITHOUT copying X: the membership pattern
## is re-indexed into X's row space; returns NULL when nothing overlaps.
.aligned_pattern <- function(X, matG) {
  G <- methods::as(methods::as(matG, "CsparseMatrix"), "generalMatrix")
  first <- !duplicated(rownames(G))
  to_x <- match(rownames(G), rownames(X))          # first match in X, NA if absent
  to_x[!first] <- NA
  if (all(is.na(to_x))) return(NULL)
  col <- rep.int(seq_len(ncol(G)), diff(G@p))
  new_i <- to_x[G@i + 1L]
  keep <- !is.na(new_i) & G@x != 0
  list(Gp = c(0L, cumsum(tabulate(col[keep], nbins = ncol(G)))),
       Gi = as.integer(new_i[keep] - 1L))
}

plaid <- function(X, matG, stats = c("mean", "sum"), chunk = NULL, normalize = TRUE) {
  stats <- stats[1]
  if (NCOL(X) == 1) X <- cbind(X)
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) {
    message("[plaid] ERROR. No overlapping features.")
    return(NULL)
  }
  .session()
  dev <- .devices()
  if (length(dev) > 1L) {                                  # sample shards over several GPUs of the node
    xa <- .x_args(X)
    S <- .Call("R_plaidhip_plaid_multi", dev, xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi,
               .stat_code(stats), normalize, PACKAGE = "plaidhip")
  } else if (inherits(X, "CsparseMatrix")) {
    S <- .Call("R_plaidhip_plaid_csc", X@p, X@i, as.double(X@x), nrow(X), pat$Gp, pat$Gi,
               .stat_code(stats), normalize, PACKAGE = "plaidhip")
  } else {
    X <- as.matrix(X); storage.mode(X) <- "double"
    S <- .Call("R_plaidhip_plaid_dense", X, pat$Gp, pat$Gi, .stat_code(stats), normalize,
               PACKAGE = "plaidhip")
  }
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

## chunked_crossprod(x, y, chunk), R/plaid.R:100-123: t(x) %*% y -- internal in the reference too.  For the
## membership matrix plaid() builds (0/1, optionally scaled per column, R/plaid.R:73-77) the column scale is read off x
## and applied to the device's unscaled sums (the scheduled membership kernels); an x whose stored values differ inside
## a column (weighted / signed sets) goes to the general sparse kernel with its @p / @i / @x slots as they are.  The
## chunk loop and its message are the reference's (the device has no 2^31 limit, the loop only bounds the size of one
## transfer).
chunked_crossprod <- function(x, y, chunk = NULL) {
  x <- methods::as(methods::as(x, "CsparseMatrix"), "generalMatrix")
  if (nrow(x) != nrow(y)) stop("non-conformable arguments")
  col <- rep.int(seq_len(ncol(x)), diff(x@p))
  nz <- x@x != 0 | is.na(x@x)
  lo <- tapply(x@x[nz], factor(col[nz], levels = seq_len(ncol(x))), min)
  hi <- tapply(x@x[nz], factor(col[nz], levels = seq_len(ncol(x))), max)
  weighted <- any(lo != hi, na.rm = TRUE) || any(!is.finite(x@x[nz]))
  if (is.null(chunk) || chunk < 0) chunk <- round(0.8 * 2147483647 / ncol(x))     # R/plaid.R:103-104
  .session()
  if (weighted) {
    Wx <- as.double(x@x)
    block <- function(jj) {
      yy <- y[, jj, drop = FALSE]
      if (inherits(yy, "CsparseMatrix")) {
        .Call("R_plaidhip_crossprod_weighted_csc", x@p, x@i, Wx, yy@p, yy@i, as.double(yy@x), nrow(yy),
              PACKAGE = "plaidhip")
      } else {
        yy <- as.matrix(yy); storage.mode(yy) <- "double"
        .Call("R_plaidhip_crossprod_weighted_dense", x@p, x@i, Wx, yy, PACKAGE = "plaidhip")
      }
    }
    scale <- 1
  } else {
    scale <- ifelse(is.na(lo), 1, lo)
    Gp <- c(0L, cumsum(tabulate(col[nz], nbins = ncol(x))))
    Gi <- x@i[nz]
    block <- function(jj) {
      yy <- y[, jj, drop = FALSE]
      if (inherits(yy, "CsparseMatrix")) {
        .Call("R_plaidhip_plaid_csc", yy@p, yy@i, as.double(yy@x), nrow(yy), Gp, Gi, 1L, FALSE, PACKAGE = "plaidhip")
      } else {
        yy <- as.matrix(yy); storage.mode(yy) <- "double"
        .Call("R_plaidhip_plaid_dense", yy, Gp, Gi, 1L, FALSE, PACKAGE = "plaidhip")
      }
    }
  }
  if (ncol(y) < chunk) {
    gsetX <- block(seq_len(ncol(y)))
  } else {
    message("[chunked_crossprod] chunked compute: chunk = ", chunk)                # R/plaid.R:109
    gsetX <- matrix(NA_real_, ncol(x), ncol(y))
    k <- ceiling(ncol(y) / chunk)
    for (i in seq_len(k)) {
      jj <- ((i - 1) * chunk + 1):min(ncol(y), i * chunk)
      gsetX[, jj] <- block(jj)
    }
  }
  gsetX <- gsetX * scale
  dimnames(gsetX) <- list(colnames(x), colnames(y))
  gsetX
}

normalize_medians <- function(x, ignore.zero = NULL) {
  .session()
  x <- as.matrix(x); storage.mode(x) <- "double"
  iz <- if (is.null(ignore.zero)) NA else as.logical(ignore.zero)
  out <- .Call("R_plaidhip_normalize_medians", x, iz, PACKAGE = "plaidhip")
  dimnames(out) <- dimnames(x)
  out
}

sparse_colranks <- function(X, signed = FALSE, ties.method = "average") {
  .session()
  X <- methods::as(X, "CsparseMatrix")
  rX <- X
  rX@x <- .Call("R_plaidhip_colranks_csc", X@p, as.double(X@x),
                .ties_code(ties.method, c("average", "first", "last", "random", "max", "min")), signed,
                PACKAGE = "plaidhip")
  rX
}

colranks <- function(X, sparse = NULL, signed = FALSE, keep.zero = FALSE, ties.method = "average") {
  if (is.null(sparse)) sparse <- inherits(X, "CsparseMatrix")
  if (sparse && keep.zero) return(sparse_colranks(X, signed = signed, ties.method = ties.method))
  .session()
  ## the `sparse` ARGUMENT picks the function (R/plaid.R:598-619): sparseMatrixStats::colRanks or matrixStats::colRanks
  code <- .ties_code(ties.method, if (sparse) c("max", "average", "min") else .ties_all)
  if (inherits(X, "CsparseMatrix") && code <= 2L) {
    ## zeros are ranked and the result is dense (sparseMatrixStats::colRanks, R/plaid.R:602-609), but the
    ## matrix goes to the device as its three CSC slots: no as.matrix(X) on the host
    rX <- .Call("R_plaidhip_colranks_csc_dense", X@p, X@i, as.double(X@x), nrow(X), code,
                signed, PACKAGE = "plaidhip")
  } else {
    D <- as.matrix(X); storage.mode(D) <- "double"
    rX <- .Call("R_plaidhip_colranks_dense", D, code, signed, PACKAGE = "plaidhip")
  }
  dimnames(rX) <- dimnames(X)
  rX
}

replaid.sing <- function(X, matG) {
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  .session()
  dev <- .devices()
  if (inherits(X, "CsparseMatrix")) {
    ## the reference densifies a sparse X to rank its zeros (R/plaid.R:602-609); here the slots go to the device(s)
    X <- methods::as(X, "generalMatrix")
    S <- if (length(dev) > 1L) .Call("R_plaidhip_sing_csc_multi", dev, X@p, X@i, as.double(X@x), nrow(X), pat$Gp, pat$Gi,
                                     PACKAGE = "plaidhip")
         else .Call("R_plaidhip_sing_csc", X@p, X@i, as.double(X@x), nrow(X), pat$Gp, pat$Gi, PACKAGE = "plaidhip")
  } else {
    D <- as.matrix(X); storage.mode(D) <- "double"
    S <- if (length(dev) > 1L) .Call("R_plaidhip_sing_multi", dev, D, pat$Gp, pat$Gi, PACKAGE = "plaidhip")
         else .Call("R_plaidhip_sing_dense", D, pat$Gp, pat$Gi, PACKAGE = "plaidhip")
  }
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

replaid.ssgsea <- function(X, matG, alpha = 0) {
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  .session()
  dev <- .devices()
  if (length(dev) > 1L) {
    xa <- .x_args(X)
    S <- .Call("R_plaidhip_ssgsea_multi", dev, xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi,
               as.double(alpha), PACKAGE = "plaidhip")
  } else if (inherits(X, "CsparseMatrix")) {
    S <- .Call("R_plaidhip_ssgsea_csc", X@p, X@i, as.double(X@x), nrow(X), pat$Gp, pat$Gi,
               as.double(alpha), PACKAGE = "plaidhip")
  } else {
    D <- as.matrix(X); storage.mode(D) <- "double"
    S <- .Call("R_plaidhip_ssgsea_dense", D, pat$Gp, pat$Gi, as.double(alpha), PACKAGE = "plaidhip")
  }
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

## X as the argument triple the shim expects: (p, i, values) for a dgCMatrix, (NULL, NULL, matrix) otherwise
.x_args <- function(X) {
  if (inherits(X, "CsparseMatrix")) list(X@p, X@i, as.double(X@x))
  else { D <- as.matrix(X); storage.mode(D) <- "double"; list(NULL, NULL, D) }
}

## The original single-sample GSEA statistic (gao.ssgsea with single = TRUE) for any alpha -- replaid.ssgsea is exact at
## alpha = 0 only (R/plaid.R:233-234, 247-248).  In closed form on the device: with average ranks r, q = rank(x,
## ties = "last") and w = r^alpha per sample, a set with k members scores sum(w q) / sum(w) - (T - sum(q)) / (N - k),
## T = N (N + 1) / 2, divided by N with scale and by diff(range(es)) of the whole result with norm.  Differs from
## gao.ssgsea on purpose in one case: a sample column holding an NA scores NA for every set, at alpha = 0 too.
## single = FALSE: the running sum's value of largest magnitude instead of its sum -- the classic GSEA enrichment score,
## step_cdf_diff[which.max(abs(step_cdf_diff))] of gao.ssgsea (first maximum, sign kept) -- from a walk kernel on the
## device (include/plaidhip.h: plaidhip_ssgsea_exact_ks); nrow(X) at most 131,072 there.
replaid.ssgsea.exact <- function(X, matG, alpha = 0.25, scale = TRUE, norm = FALSE, single = TRUE) {
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  .session()
  if (!isTRUE(as.logical(single))) return(.ssgsea_exact_ks(X, matG, pat, alpha, scale, norm))
  xa <- .x_args(X)
  dev <- .devices()
  S <- if (length(dev) > 1L) .Call("R_plaidhip_ssgsea_exact_multi", dev, xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X),
                                   pat$Gp, pat$Gi, as.double(alpha), as.logical(scale), as.logical(norm), PACKAGE = "plaidhip")
       else .Call("R_plaidhip_ssgsea_exact", xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi, as.double(alpha),
                  as.logical(scale), as.logical(norm), PACKAGE = "plaidhip")
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

.ssgsea_exact_ks <- function(X, matG, pat, alpha, scale, norm) {
  xa <- .x_args(X)
  dev <- .devices()
  S <- if (length(dev) > 1L) .Call("R_plaidhip_ssgsea_exact_ks_multi", dev, xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X),
                                   pat$Gp, pat$Gi, as.double(alpha), as.logical(scale), as.logical(norm), PACKAGE = "plaidhip")
       else .Call("R_plaidhip_ssgsea_exact_ks", xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi, as.double(alpha),
                  as.logical(scale), as.logical(norm), PACKAGE = "plaidhip")
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

replaid.ucell <- function(X, matG, rmax = 1500) {
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  .session()
  xa <- .x_args(X)
  kfull <- as.double(Matrix::colSums(matG != 0))
  dev <- .devices()
  S <- if (length(dev) > 1L) .Call("R_plaidhip_ucell_multi", dev, xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp,
                                   pat$Gi, kfull, as.double(rmax), PACKAGE = "plaidhip")
       else .Call("R_plaidhip_ucell", xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi, kfull, as.double(rmax),
                  PACKAGE = "plaidhip")
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

replaid.aucell <- function(X, matG, aucMaxRank = ceiling(0.05 * nrow(X))) {
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  .session()
  xa <- .x_args(X)
  dev <- .devices()
  S <- if (length(dev) > 1L) .Call("R_plaidhip_aucell_multi", dev, xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp,
                                   pat$Gi, as.double(aucMaxRank), PACKAGE = "plaidhip")
       else .Call("R_plaidhip_aucell", xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi, as.double(aucMaxRank),
                  PACKAGE = "plaidhip")
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

## UCell's statistic on truncated ranks -- replaid.ucell (R/plaid.R:276-282) is "near exact": max(rX) - rX for the descending
## rank, plaid()'s median normalisation and its 1e-8.  The formulas follow UCell AS RECALLED (the package's source is not in
## this tree); include/plaidhip.h (plaidhip_ucell_exact) pins them: per sample d = rank(-x, ties = "average") over ALL rows
## of X, truncated by UCell's rule c = (d <= maxRank) ? d : maxRank + 1 (not pmin: a tie group is kept as a whole or not at
## all); for a set of K members 1 - U / (K maxRank) with U = sum(c) - K (K + 1) / 2, formed in integers and closed by one
## division.  K is the number of aligned members, or with impute = TRUE colSums(matG != 0) of the un-aligned matrix (UCell's
## missing_genes = "impute": absent members count with rank maxRank + 1); k_full overrides it for the up sets.  matD
## (optional): the down sets, column j pairing with column j of matG; TotalScore = UpScore - w_neg * DownScore, below 0
## gives 0.  Sets without members score NA; an empty down column makes its TotalScore NA; a sample holding an NA is NA
## everywhere.  No normalize_medians.  A dgCMatrix is never expanded, on the host or on the device.  Returns a list of sets x
## samples matrices: UpScore and, with matD, TotalScore and DownScore.  options(plaidhip.devices = ...) shards the samples.
replaid.ucell.exact <- function(X, matG, matD = NULL, maxRank = 1500, w_neg = 1, k_full = NULL, impute = FALSE) {
  if (!is.null(matD) && ncol(matD) != ncol(matG)) stop("ucell_exact: matD has ", ncol(matD), " columns, matG ", ncol(matG))
  maxRank <- as.double(maxRank); w_neg <- as.double(w_neg)
  if (length(maxRank) != 1L || is.na(maxRank) || maxRank != floor(maxRank) || maxRank < 1 || maxRank > nrow(X))
    stop("ucell_exact: maxRank must be an integer in 1..nrow(X)")
  if (length(w_neg) != 1L || !is.finite(w_neg) || w_neg < 0) stop("ucell_exact: w_neg must be finite and >= 0")
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  Dp <- integer(0); Di <- integer(0)
  if (!is.null(matD)) {
    dpat <- .aligned_pattern(X, matD)
    if (is.null(dpat)) dpat <- list(Gp = integer(ncol(matD) + 1L), Gi = integer(0))
    Dp <- dpat$Gp; Di <- dpat$Gi
  }
  kf <- double(0); kd <- double(0)
  if (!is.null(k_full) || isTRUE(impute)) {
    kf <- if (!is.null(k_full)) as.double(k_full) else as.double(Matrix::colSums(matG != 0))
    if (length(kf) != ncol(matG)) stop("ucell_exact: k_full must have one entry per set")
    if (!is.null(matD)) kd <- as.double(Matrix::colSums(matD != 0))
  }
  .session()
  if (methods::is(X, "sparseMatrix")) X <- methods::as(X, "generalMatrix")
  xa <- .x_args(X)
  dev <- .devices()
  res <- .Call("R_plaidhip_ucell_exact", if (length(dev) > 1L) dev else integer(0), xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X),
               pat$Gp, pat$Gi, Dp, Di, maxRank, w_neg, kf, kd, PACKAGE = "plaidhip")
  names(res) <- c("TotalScore", "UpScore", "DownScore")
  res <- res[!vapply(res, is.null, logical(1))]
  lapply(res, function(S) { dimnames(S) <- list(colnames(matG), colnames(X)); S })
}

## AUCell's AUC on truncated ranks -- replaid.aucell (R/plaid.R:304-309) is a ramp with a factor of 1.08.  The formulas
## follow AUCell AS RECALLED; include/plaidhip.h (plaidhip_aucell_exact) pins them: per sample the positions
## pos = N + 1 - rank(x, ties = "last") over ALL rows of X (AUCell breaks ties at random; here the earlier row comes first, so
## that the result is a function of its input); area = sum(aucMaxRank - pos) over the members with pos < aucMaxRank,
## divided by the largest area min(k, aucMaxRank - 1) members can reach.  Sets without aligned members score NA, as does
## aucMaxRank = 1.  No normalize_medians; random ties and AUCell's older normalisation (aucMaxRank * k) are not offered.  A
## dgCMatrix is never expanded.  options(plaidhip.devices = ...) shards the samples.
replaid.aucell.exact <- function(X, matG, aucMaxRank = ceiling(0.05 * nrow(X))) {
  aucMaxRank <- as.double(aucMaxRank)
  if (length(aucMaxRank) != 1L || is.na(aucMaxRank) || aucMaxRank != floor(aucMaxRank) || aucMaxRank < 1 ||
      aucMaxRank > nrow(X)) stop("aucell_exact: aucMaxRank must be an integer in 1..nrow(X)")
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  .session()
  if (methods::is(X, "sparseMatrix")) X <- methods::as(X, "generalMatrix")
  xa <- .x_args(X)
  dev <- .devices()
  S <- .Call("R_plaidhip_aucell_exact", if (length(dev) > 1L) dev else integer(0), xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X),
             pat$Gp, pat$Gi, aucMaxRank, PACKAGE = "plaidhip")
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

replaid.scse <- function(X, matG, removeLog2 = NULL, scoreMean = FALSE) {
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  .session()
  xa <- .x_args(X)
  rl <- if (is.null(removeLog2)) NA else as.logical(removeLog2)
  dev <- .devices()
  S <- if (length(dev) > 1L) .Call("R_plaidhip_scse_multi", dev, xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp,
                                   pat$Gi, rl, as.logical(scoreMean), PACKAGE = "plaidhip")
       else .Call("R_plaidhip_scse", xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi, rl, as.logical(scoreMean),
                  PACKAGE = "plaidhip")
  if (isTRUE(attr(S, "removedLog2")))   ## R/plaid.R:163-164 (the NULL case is decided on the device)
    message("[replaid.scse] Converting data to linear scale (removing log2)...")
  attr(S, "removedLog2") <- NULL
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}


## gmt2mat(read.gmt(file)) as ONE native call (the text never becomes an R list): same ordering rules
## as R/gmt-utils.R:19-66 (sets by size, duplicated names dropped, head(ntop), genes by frequency,
## head(max.genes), rows by decreasing row sum).  50k sets: ~2 s instead of ~50 s.
gmt2mat.file <- function(gmt.file, dir = NULL, add.source = FALSE, nrows = -1,
                         max.genes = -1, ntop = -1, sparse = TRUE, bg = NULL) {
  f0 <- gmt.file
  if (strtrim(gmt.file, 1) == "/") dir <- NULL
  if (!is.null(dir)) f0 <- paste(sub("/$", "", dir), "/", gmt.file, sep = "")
  r <- .Call("R_plaidhip_gmt2mat_file", f0, add.source, nrows, max.genes, ntop, bg, PACKAGE = "plaidhip")
  D <- methods::new("dgCMatrix", p = r[[1]], i = r[[2]], x = rep(1, length(r[[2]])), Dim = r[[3]],
                    Dimnames = list(r[[4]], r[[5]]))
  if (!sparse) D <- as.matrix(D)
  D
}


## plaid.test(), R/plaid.R:392-474: same arguments and result; the group means of X, Gt fc, Gt fc^2 and the
## per-set Welch statistics are reduced on the device (with gsetX = NULL the score matrix never leaves it),
## only O(sets) numbers come back.
plaid.test <- function(X, y, G, gsetX, tests = c("one", "two", "lm"),
                       metap.method = "fisher", sort.by = "p.meta") {
  ## (the reference's signature, R/plaid.R:392: gsetX has no default; left out, it is recomputed from X and G like NULL)
  if (missing(gsetX)) gsetX <- NULL
  if (!all(unique(y) %in% c(0, 1))) stop("elements of y must be 0 or 1")
  if (is.list(G)) {
    message("[plaid.test] converting gmt to sparse matrix...")
    G <- gmt2mat(G)
  }
  if (!metap.method %in% c("fisher", "sumlog", "stouffer", "sumz")) stop("Invalid method: ", metap.method)
  gg <- intersect(rownames(G), rownames(X))
  sparse <- inherits(X, "CsparseMatrix")
  if (sparse) {
    X <- methods::as(X[gg, , drop = FALSE], "generalMatrix")   # stays a dgCMatrix: its slots go to the device
  } else {
    X <- as.matrix(X[gg, , drop = FALSE]); storage.mode(X) <- "double"
  }
  G <- G[gg, , drop = FALSE]
  pat <- .aligned_pattern(X, G)                           # stored zeros of G are dropped: set sizes count members only
  if (!is.null(gsetX)) { gsetX <- as.matrix(gsetX[colnames(G), , drop = FALSE]); storage.mode(gsetX) <- "double" }
  bits <- sum(c(one = 1L, two = 2L, lm = 4L)[intersect(tests, c("one", "two", "lm"))])
  .session()
  mm <- as.integer(metap.method %in% c("stouffer", "sumz"))
  dev <- .devices()
  r <- if (length(dev) > 1L) {
         ## sample shards over several GPUs: the scores stay on them, only per-gene and per-set sums are combined
         xa <- .x_args(X)
         .Call("R_plaidhip_plaid_test_multi", dev, xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), as.integer(y), pat$Gp,
               pat$Gi, gsetX, bits, mm, PACKAGE = "plaidhip")
       } else if (sparse) .Call("R_plaidhip_plaid_test_csc", X@p, X@i, as.double(X@x), nrow(X), as.integer(y), pat$Gp,
                                pat$Gi, gsetX, bits, mm, PACKAGE = "plaidhip")
       else .Call("R_plaidhip_plaid_test", X, as.integer(y), pat$Gp, pat$Gi, gsetX, bits, mm, PACKAGE = "plaidhip")
  keep <- c(TRUE, "one" %in% tests, "two" %in% tests, "lm" %in% tests, TRUE, TRUE)
  res <- r[, keep, drop = FALSE]
  dimnames(res) <- list(colnames(G), c("gsetFC", "p.one", "p.two", "p.lm", "p.meta", "q.meta")[keep])
  if (sort.by %in% colnames(res)) res <- res[order(res[, sort.by]), ]
  res
}


## plaid.test.contrasts(): plaid.test() for every column of a contrast matrix Y (samples x contrasts; 0, 1, NA = the sample
## takes no part) in ONE call.  Contrast j is plaid.test(X[, sel], Y[sel, j], G, gsetX = S[, sel]) with sel <- !is.na(Y[, j])
## and S the gsetX given or plaid(X, G) over all samples, computed once; every pass over the scores is shared by the
## contrasts.  Returns a named list (the columns of Y) of plaid.test() results.
plaid.test.contrasts <- function(X, Y, G, gsetX = NULL, tests = c("one", "two", "lm"),
                                 metap.method = "fisher", sort.by = "p.meta") {
  Y <- as.matrix(Y)
  if (nrow(Y) != ncol(X)) stop("Y must have one row per column of X")
  if (!all(unique(as.vector(Y)) %in% c(0, 1, NA))) stop("elements of Y must be 0, 1 or NA")
  if (is.list(G)) {
    message("[plaid.test] converting gmt to sparse matrix...")
    G <- gmt2mat(G)
  }
  if (!metap.method %in% c("fisher", "sumlog", "stouffer", "sumz")) stop("Invalid method: ", metap.method)
  gg <- intersect(rownames(G), rownames(X))
  sparse <- inherits(X, "CsparseMatrix")
  if (sparse) {
    X <- methods::as(X[gg, , drop = FALSE], "generalMatrix")
  } else {
    X <- as.matrix(X[gg, , drop = FALSE]); storage.mode(X) <- "double"
  }
  G <- G[gg, , drop = FALSE]
  pat <- .aligned_pattern(X, G)
  if (!is.null(gsetX)) { gsetX <- as.matrix(gsetX[colnames(G), , drop = FALSE]); storage.mode(gsetX) <- "double" }
  bits <- sum(c(one = 1L, two = 2L, lm = 4L)[intersect(tests, c("one", "two", "lm"))])
  .session()
  mm <- as.integer(metap.method %in% c("stouffer", "sumz"))
  Yi <- matrix(as.integer(Y), nrow(Y), ncol(Y))
  Yi[is.na(Yi)] <- -1L
  xa <- .x_args(X)
  r <- .Call("R_plaidhip_plaid_test_contrasts", .devices(), xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), Yi, pat$Gp, pat$Gi,
             gsetX, bits, mm, PACKAGE = "plaidhip")
  dim(r) <- c(nrow(r), 6L, ncol(Y))
  keep <- c(TRUE, "one" %in% tests, "two" %in% tests, "lm" %in% tests, TRUE, TRUE)
  cn <- if (is.null(colnames(Y))) as.character(seq_len(ncol(Y))) else colnames(Y)
  out <- lapply(seq_len(ncol(Y)), function(j) {
    res <- matrix(r[, keep, j], nrow = dim(r)[1])
    dimnames(res) <- list(colnames(G), c("gsetFC", "p.one", "p.two", "p.lm", "p.meta", "q.meta")[keep])
    if (sort.by %in% colnames(res)) res <- res[order(res[, sort.by]), , drop = FALSE]
    res
  })
  names(out) <- cn
  out
}


## plaid.gsea(): preranked GSEA with a permutation null on the device -- what fgsea::fgsea(gmt, fc) gives the enrichment
## experiments (experiments/compare-enrichment/enrichment-methods.R:28): ES, NES, pval, padj for a named vector of
## statistics, or for every column of a genes x contrasts matrix.  include/plaidhip.h (plaidhip_gsea) pins the statistic
## (fgseaSimple); the weights abs(stats)^gseaParam are formed here.  perm: NULL (nperm placements
## generated from seed) or a genes x nperm integer matrix whose columns are permutations of seq_len(genes) over the aligned
## genes.  Returns a matrix (a vector of statistics) or a named list of matrices, rows ordered by sort.by.
## scoreType "pos" / "neg" scores one side of the walk (a statistic of one sign: |logFC|, F, -log p).  leadingEdge = TRUE
## returns, wherever a matrix is returned, list(table = <that matrix>, leadingEdge = <named list, one character vector of
## gene names per table row in the table's order: the genes that drive the set's score, in walk order>).
## multilevel = TRUE (fgsea's multilevel reading, as pinned in include/plaidhip.h: plaidhip_gsea_multilevel) replaces the pval
## of every set that fewer than mlMin permutations matched by an adaptive multilevel splitting estimate from sampleSize
## chains (odd), sweeps * size proposals a stage, down to about eps; padj is over the reported pval and the table gains a
## log2err column (NA where the permutation pval stands).
plaid.gsea <- function(stats, G, nperm = 1000, gseaParam = 1, minSize = 1, maxSize = NULL, seed = 1, perm = NULL,
                       sort.by = "pval", scoreType = c("std", "pos", "neg"), leadingEdge = FALSE, multilevel = FALSE,
                       sampleSize = 101, eps = 1e-50, sweeps = 4, mlMin = 10) {
  scoreType <- match.arg(scoreType)
  single <- is.null(dim(stats))
  if (single) stats <- matrix(stats, ncol = 1, dimnames = list(names(stats), "stat"))
  stats <- as.matrix(stats); storage.mode(stats) <- "double"
  if (is.list(G)) {
    message("[plaid.gsea] converting gmt to sparse matrix...")
    G <- gmt2mat(G)
  }
  if (length(gseaParam) != 1L || !is.finite(gseaParam) || gseaParam < 0) stop("plaid.gsea: gseaParam must be finite and >= 0")
  gg <- intersect(rownames(G), rownames(stats))
  stats <- stats[gg, , drop = FALSE]
  G <- G[gg, , drop = FALSE]
  size <- Matrix::colSums(G != 0)
  if (is.null(maxSize)) maxSize <- length(gg) - 1L
  G <- G[, size >= minSize & size <= maxSize, drop = FALSE]
  pat <- .aligned_pattern(stats, G)
  W <- abs(stats)^gseaParam
  W[!is.finite(W)] <- 0
  if (!is.null(perm)) {
    perm <- as.matrix(perm)
    if (nrow(perm) != nrow(stats)) stop("plaid.gsea: perm must have one row per aligned gene")
    perm <- matrix(as.integer(perm) - 1L, nrow(perm), ncol(perm))
  }
  .session()
  edges <- isTRUE(as.logical(leadingEdge))
  le <- NULL
  ml <- NULL
  if (isTRUE(as.logical(multilevel))) {
    le <- .Call("R_plaidhip_gsea_multilevel", .devices(), stats, W, pat$Gp, pat$Gi, perm, as.integer(nperm),
                as.numeric(seed %% 2^32), as.numeric((seed %/% 2^32) %% 2^32), match(scoreType, c("std", "pos", "neg")) - 1L,
                edges, as.numeric(c(sampleSize, sweeps, eps, mlMin)), PACKAGE = "plaidhip")
    r <- le[[1]]
    ml <- le[[4]]
    dim(ml) <- c(nrow(ml), 6L, ncol(stats))
  } else if (scoreType == "std" && !edges) {
    r <- .Call("R_plaidhip_gsea", .devices(), stats, W, pat$Gp, pat$Gi, perm, as.integer(nperm), as.numeric(seed %% 2^32),
               as.numeric((seed %/% 2^32) %% 2^32), PACKAGE = "plaidhip")
  } else {
    le <- .Call("R_plaidhip_gsea_scored", .devices(), stats, W, pat$Gp, pat$Gi, perm, as.integer(nperm),
                as.numeric(seed %% 2^32), as.numeric((seed %/% 2^32) %% 2^32), match(scoreType, c("std", "pos", "neg")) - 1L,
                edges, PACKAGE = "plaidhip")
    r <- le[[1]]
  }
  dim(r) <- c(nrow(r), 12L, ncol(stats))
  cols <- c("ES", "NES", "pval", "padj", "nMoreExtreme", "size")
  out <- lapply(seq_len(ncol(stats)), function(l) {
    res <- matrix(r[, 1:6, l], nrow = dim(r)[1], dimnames = list(colnames(G), cols))
    if (!is.null(ml)) res <- cbind(res, log2err = ifelse(!is.na(r[, 5, l]) & r[, 5, l] < mlMin, ml[, 2, l], NA_real_))
    o <- if (sort.by %in% cols) order(res[, sort.by]) else seq_len(nrow(res))
    res <- res[o, , drop = FALSE]
    if (!edges) return(res)
    ## the edge of set j in list l: le_idx[Gp[j] + seq_len(le_len[j, l]), l], 0-based rows of the aligned genes
    led <- lapply(o, function(j) rownames(stats)[le[[3]][pat$Gp[j] + seq_len(le[[2]][j, l]), l] + 1L])
    names(led) <- rownames(res)
    list(table = res, leadingEdge = led)
  })
  names(out) <- colnames(stats)
  if (single) out[[1]] else out
}


## plaid.sig(): the lists plaid.fisher() takes, from gene-level results, by the rule of the enrichment experiments
## (experiments/compare-enrichment/enrichment-methods.R:22-23): +1 where logFC > lfc & pvalue < pcut, -1 where
## logFC < -lfc & pvalue < pcut, 0 elsewhere (an NA in either input gives 0).  logFC and pvalue: vectors or matrices of
## one shape; the names of logFC are kept.  Runs on the host.
plaid.sig <- function(logFC, pvalue, lfc = 0.2, pcut = 0.05) {
  if (!identical(dim(logFC), dim(pvalue)) || length(logFC) != length(pvalue)) stop("plaid.sig: logFC and pvalue must have one shape")
  hit <- !is.na(pvalue) & !is.na(logFC) & pvalue < pcut
  s <- logFC
  s[] <- 0L
  s[hit & logFC > lfc] <- 1L
  s[hit & logFC < -lfc] <- -1L
  storage.mode(s) <- "integer"
  s
}


## plaid.fisher(): over-representation analysis on the device -- what gset.fisher2(sig.up, sig.dn, gmt) gives the enrichment
## experiments (experiments/compare-enrichment/enrichment-methods.R:29): Fisher's exact (hypergeometric, upper tail) test of
## the genes significant up, down and either way against every set, for a named vector of -1 / 0 / 1 (plaid.sig makes one)
## or for every column of a genes x contrasts matrix.  include/plaidhip.h (plaidhip_fisher) pins the statistic.  Genes are
## aligned by name as plaid.gsea aligns them; the universe is the aligned rows.  Returns a matrix (a vector) or a named list
## of matrices: sets x (size, ovUp, ovDn, pUp, pDn, pAny, padjUp, padjDn, padjAny, orUp, orDn, orAny), rows ordered by
## sort.by (NA last).  overlap = TRUE returns, wherever a matrix is returned, list(table = <that matrix>, overlap = <named
## list, one named integer vector per table row in the table's order: the sign of every member of the set that is in the
## list, named by gene, in the set's member order>).
plaid.fisher <- function(sig, G, minSize = 1, maxSize = NULL, sort.by = "pAny", overlap = FALSE) {
  single <- is.null(dim(sig))
  if (single) sig <- matrix(sig, ncol = 1, dimnames = list(names(sig), "sig"))
  sig <- as.matrix(sig)
  if (anyNA(sig) || !all(sig %in% c(-1, 0, 1))) stop("plaid.fisher: sig must hold -1, 0 or 1")
  storage.mode(sig) <- "integer"
  if (is.list(G)) {
    message("[plaid.fisher] converting gmt to sparse matrix...")
    G <- gmt2mat(G)
  }
  gg <- intersect(rownames(G), rownames(sig))
  sig <- sig[gg, , drop = FALSE]
  G <- G[gg, , drop = FALSE]
  size <- Matrix::colSums(G != 0)
  if (is.null(maxSize)) maxSize <- length(gg) - 1L
  G <- G[, size >= minSize & size <= maxSize, drop = FALSE]
  pat <- .aligned_pattern(sig, G)
  .session()
  want <- isTRUE(as.logical(overlap))
  r <- .Call("R_plaidhip_fisher", .devices(), sig, pat$Gp, pat$Gi, want, PACKAGE = "plaidhip")
  tab <- r[[1]]
  dim(tab) <- c(nrow(tab), 12L, ncol(sig))
  cols <- c("size", "ovUp", "ovDn", "pUp", "pDn", "pAny", "padjUp", "padjDn", "padjAny", "orUp", "orDn", "orAny")
  out <- lapply(seq_len(ncol(sig)), function(l) {
    res <- matrix(tab[, , l], nrow = dim(tab)[1], dimnames = list(colnames(G), cols))
    o <- if (sort.by %in% cols) order(res[, sort.by]) else seq_len(nrow(res))
    res <- res[o, , drop = FALSE]
    if (!want) return(res)
    ## the overlap of set j in list l: ov_idx[Gp[j] + seq_len(ov_len[j, l]), l], 0-based rows of the aligned genes
    ov <- lapply(o, function(j) {
      rows <- r[[4]][pat$Gp[j] + seq_len(r[[3]][j, l]), l] + 1L
      stats::setNames(sig[rows, l], rownames(sig)[rows])
    })
    names(ov) <- rownames(res)
    list(table = res, overlap = ov)
  })
  names(out) <- colnames(sig)
  if (single) out[[1]] else out
}


## plaid.rankcor(): the reference's gset.rankcor(fc, matG, compute.p = TRUE) (experiments/R/functions.R:183-237) on the device
## -- the "rankcor" and (use.rank = FALSE) "cor" families of the enrichment experiments
## (experiments/compare-enrichment/enrichment-methods.R:36-37) and the first two single-sample scorers of run.methods: the
## Pearson correlation of the ranks of a per-gene statistic, or of the statistic itself, with the 0/1 membership of every
## set, for a named vector or every column of a genes x lists matrix (contrasts, or samples).  An NA leaves the gene out of
## that list alone (ranks with na.last = "keep"; the universe and the set sizes are the list's own).
## include/plaidhip.h (plaidhip_rankcor) pins the statistic.  ties: "average" (default), "min" or "max"; the reference's
## ties.method = "random" is no function of the input and is not offered (lists without ties are the same under all of
## them).  Genes are aligned by name as plaid.gsea aligns them.  Returns a matrix (a vector) or a named list of matrices:
## sets x (size, rho, t, p.value, q.value) -- (size, rho) with compute.p = FALSE -- rows ordered by sort.by (NA last;
## decreasing |rho| for "rho").
plaid.rankcor <- function(stat, G, use.rank = TRUE, compute.p = TRUE, ties = c("average", "min", "max"), minSize = 1,
                          maxSize = NULL, sort.by = "p.value") {
  ties <- match.arg(ties)
  single <- is.null(dim(stat))
  if (single) stat <- matrix(stat, ncol = 1, dimnames = list(names(stat), "stat"))
  stat <- as.matrix(stat); storage.mode(stat) <- "double"
  if (is.list(G)) {
    message("[plaid.rankcor] converting gmt to sparse matrix...")
    G <- gmt2mat(G)
  }
  gg <- intersect(rownames(G), rownames(stat))
  stat <- stat[gg, , drop = FALSE]
  G <- G[gg, , drop = FALSE]
  size <- Matrix::colSums(G != 0)
  if (is.null(maxSize)) maxSize <- length(gg) - 1L
  G <- G[, size >= minSize & size <= maxSize, drop = FALSE]
  pat <- .aligned_pattern(stat, G)
  .session()
  r <- .Call("R_plaidhip_rankcor", .devices(), stat, pat$Gp, pat$Gi, isTRUE(as.logical(use.rank)),
             match(ties, c("average", "min", "max")) - 1L, PACKAGE = "plaidhip")
  tab <- r[[1]]
  dim(tab) <- c(nrow(tab), 5L, ncol(stat))
  cols <- c("size", "rho", "t", "p.value", "q.value")
  if (!isTRUE(as.logical(compute.p))) cols <- cols[1:2]
  out <- lapply(seq_len(ncol(stat)), function(l) {
    res <- matrix(tab[, seq_along(cols), l], nrow = dim(tab)[1], dimnames = list(colnames(G), cols))
    o <- if (sort.by %in% cols) order(if (sort.by == "rho") -abs(res[, "rho"]) else res[, sort.by]) else seq_len(nrow(res))
    res[o, , drop = FALSE]
  })
  names(out) <- colnames(stat)
  if (single) out[[1]] else out
}


## the tables of plaid.limma() / plaid.limma.contrasts() from the library's rows x 6 block: topTable's order for sort.by --
## "none" (the rows of S), "P.Value" / "P" / "p" (increasing), "t" and "logFC" (decreasing magnitude), "AveExpr" (decreasing)
.limma_sorts <- c("none", "P.Value", "P", "p", "t", "logFC", "AveExpr")

.limma_table <- function(tab, rn, sort.by, dfr = NULL) {
  cols <- c("logFC", "AveExpr", "t", "P.Value", "adj.P.Val", "sigma2")
  res <- matrix(tab, nrow = length(rn), ncol = 6L, dimnames = list(rn, cols))
  if (!is.null(dfr)) {   # na = "fit": the rows' own df.residual, NA where the row is NA
    dfr[is.na(res[, "sigma2"])] <- NA_real_
    res <- cbind(res, df.residual = dfr)
  }
  key <- switch(sort.by, none = NULL, P.Value = , P = , p = res[, "P.Value"], t = -abs(res[, "t"]),
                logFC = -abs(res[, "logFC"]), AveExpr = -res[, "AveExpr"],
                stop("plaid.limma: sort.by must be one of ", paste(.limma_sorts, collapse = ", ")))
  if (!is.null(key)) res <- res[order(key), , drop = FALSE]
  res
}

.limma_hyper <- function(h) stats::setNames(as.list(h), c("df.residual", "df.prior", "s2.prior", "n.ok", "df.pooled")[seq_along(h)])

## weights of plaid.limma() as the shim takes them: list(Wt, aw), a double matrix in S's shape or NULL and a double vector
## over the samples or NULL
.limma_weights <- function(S, weights) {
  if (is.null(weights)) return(NULL)
  if (is.matrix(weights) || is.data.frame(weights)) {
    weights <- as.matrix(weights); storage.mode(weights) <- "double"
    if (!identical(dim(weights), dim(S))) stop("plaid.limma: a matrix of weights has the shape of S")
    return(list(weights, NULL))
  }
  if (length(weights) != ncol(S)) stop("plaid.limma: a vector of weights has one entry per sample")
  list(NULL, as.double(weights))
}

## the library call behind both: na = "propagate" is plaidhip_limma; na = "fit" is plaidhip_limma_na, whose tables get the
## rows' own df.residual as a seventh column (NA where the row is NA); with weights plaidhip_limma_w, whose result is that of
## na = "fit" (na = "propagate" then stands for max.na = 0: no row with an NA is fitted)
.limma_call <- function(S, D, nfit, use, K, na, max.na, ncon, rn, sort.by, weights = NULL) {
  if (!is.null(weights)) {
    if (na == "propagate") max.na <- 0
    if (length(max.na) != 1L || is.na(max.na) || max.na < 0 || max.na > 1) stop("plaid.limma: max.na must be a share in [0, 1]")
    r <- .Call("R_plaidhip_limma_w", .devices(), S, weights[[1]], weights[[2]], D, nfit, use, K, as.double(max.na),
               PACKAGE = "plaidhip")
    na <- "fit"
  } else if (na == "propagate") {
    r <- .Call("R_plaidhip_limma", .devices(), S, D, nfit, use, K, PACKAGE = "plaidhip")
  } else {
    if (length(max.na) != 1L || is.na(max.na) || max.na < 0 || max.na > 1) stop("plaid.limma: max.na must be a share in [0, 1]")
    r <- .Call("R_plaidhip_limma_na", .devices(), S, D, nfit, use, K, as.double(max.na), PACKAGE = "plaidhip")
  }
  out <- r[[1]]
  dim(out) <- c(nrow(S), 6L, ncon)
  tables <- lapply(seq_len(ncon), function(j)
    .limma_table(out[, , j], rn, sort.by, if (na == "fit") r[[3]][, if (nfit == 1L) 1L else j] else NULL))
  list(tables = tables, hyper = r[[2]])
}


## plaid.limma(): limma's moderated t-test (lmFit + eBayes + topTable, as pinned in include/plaidhip.h: plaidhip_limma) of
## every row of S -- single-sample scores (sets x samples) or expression (genes x samples) -- for one design (samples x
## coefficients).  contrasts: coefficients x contrasts, NULL: every coefficient.  use: one entry per sample, FALSE / 0 / NA
## leaves it out of the fit.  Returns list(tables = <named list, one matrix per contrast: rows x (logFC, AveExpr, t, P.Value,
## adj.P.Val, sigma2), ordered by sort.by>, hyper = list(df.residual, df.prior, s2.prior, n.ok)).  logFC and P.Value are what
## plaid.sig() and plaid.gsea() take.  na = "propagate": an NA in a used sample makes the row NA.  na = "fit": limma's own
## handling -- a row with at most the share max.na of NA over all samples (gx.limma's max.na) is refitted on the samples it
## has, with its own df.residual (a seventh column of the tables) and stdev.unscaled, and eBayes takes the unequal df
## (hyper gains df.pooled); a row above max.na, or not estimable on what it has, is NA; at most 10 coefficients.
## weights: NULL, a matrix in S's shape (observation weights, limma's `weights`: voom's, or quality weights from upstream) or a
## vector over the samples (array weights): the weighted least squares of every row (plaidhip_limma_w).  An observation with
## an NA value or a weight that is zero, negative, NA or infinite is missing, as in limma; the tables are those of na = "fit"
## (na = "propagate" then fits no row that holds an NA); at most 10 coefficients.
## Not offered: trend, robust, the B- and F-statistics, a sparse S; weights in the set tests.
plaid.limma <- function(S, design, contrasts = NULL, use = NULL, sort.by = "none", na = c("propagate", "fit"), max.na = 0.2,
                        weights = NULL) {
  na <- match.arg(na)
  S <- as.matrix(S); storage.mode(S) <- "double"
  design <- as.matrix(design); storage.mode(design) <- "double"
  if (nrow(design) != ncol(S)) stop("design must have one row per column of S")
  cn <- if (is.null(colnames(design))) paste0("coef", seq_len(ncol(design))) else colnames(design)
  if (!is.null(contrasts)) {
    contrasts <- as.matrix(contrasts); storage.mode(contrasts) <- "double"
    if (nrow(contrasts) != ncol(design)) stop("contrasts must have one row per coefficient")
    cn <- if (is.null(colnames(contrasts))) as.character(seq_len(ncol(contrasts))) else colnames(contrasts)
  }
  if (!is.null(use)) {
    if (length(use) != ncol(S)) stop("use must have one entry per column of S")
    use <- matrix(as.integer(!is.na(use) & use != 0), ncol = 1)
  }
  rn <- if (is.null(rownames(S))) paste0("row", seq_len(nrow(S))) else rownames(S)
  if (length(sort.by) != 1L || !sort.by %in% .limma_sorts) stop("plaid.limma: sort.by must be one of ", paste(.limma_sorts, collapse = ", "))
  weights <- .limma_weights(S, weights)
  .session()
  r <- .limma_call(S, design, 1L, use, contrasts, na, max.na, length(cn), rn, sort.by, weights)
  tables <- r$tables
  names(tables) <- cn
  list(tables = tables, hyper = .limma_hyper(r$hyper[, 1]))
}


## plaid.voom(): limma's voom with normalize.method = "none" (as pinned in include/plaidhip.h: plaidhip_voom) of a counts matrix
## (genes x samples, finite and >= 0) for one design.  lib.size: one entry per sample, NULL: the column sums.  span: the lowess
## span of the mean-variance trend.  Returns list(E = <log2-CPM>, weights = <precision weights>, lib.size, offset =
## log2(lib.size + 1) - log2(1e6), knots.x, knots.y = <the trend's knots>); plaid.limma(v$E, design, weights = v$weights) is
## limma's lmFit + eBayes on that EList.  Not offered: other normalize.method, voomWithQualityWeights, arrayWeights,
## duplicateCorrelation, a dgCMatrix of counts.
plaid.voom <- function(counts, design, lib.size = NULL, span = 0.5) {
  counts <- as.matrix(counts); storage.mode(counts) <- "double"
  design <- as.matrix(design); storage.mode(design) <- "double"
  if (nrow(design) != ncol(counts)) stop("design must have one row per column of counts")
  if (!is.null(lib.size)) {
    if (length(lib.size) != ncol(counts)) stop("lib.size must have one entry per column of counts")
    lib.size <- as.double(lib.size)
  }
  if (length(span) != 1L || is.na(span) || span <= 0 || span > 1) stop("plaid.voom: span must lie in (0, 1]")
  .session()
  r <- .Call("R_plaidhip_voom", .devices(), counts, design, lib.size, as.double(span), PACKAGE = "plaidhip")
  names(r) <- c("E", "weights", "lib.size", "offset", "knots.x", "knots.y")
  dimnames(r$E) <- dimnames(r$weights) <- dimnames(counts)
  names(r$lib.size) <- names(r$offset) <- colnames(counts)
  r
}


## plaid.limma.contrasts(): gx.limma(S, y, B, method = 1) (experiments/R/functions.R:294-444) for every column of a contrast
## matrix Y (samples x contrasts; 0, 1, NA = the sample takes no part) in ONE call: contrast j fits [1, Y[, j], B] on the
## samples with a label and tests the coefficient of Y[, j].  B: batch covariates (samples x covariates) or NULL.  S is
## uploaded once and read ceiling(ncol(Y) * (p + 1) / 8) times for the effects.  Returns list(tables = <named list (the
## columns of Y) of plaid.limma() tables>, hyper = <named list of their hyper-parameters>).  na, max.na: as plaid.limma();
## na = "fit" with max.na = 0.2 is gx.limma(S, y, B, max.na = 0.20) on a matrix with missing values.  weights: as plaid.limma(),
## shared by the contrasts.
plaid.limma.contrasts <- function(S, Y, B = NULL, sort.by = "none", na = c("propagate", "fit"), max.na = 0.2, weights = NULL) {
  na <- match.arg(na)
  S <- as.matrix(S); storage.mode(S) <- "double"
  Y <- as.matrix(Y)
  if (nrow(Y) != ncol(S)) stop("Y must have one row per column of S")
  if (!all(unique(as.vector(Y)) %in% c(0, 1, NA))) stop("elements of Y must be 0, 1 or NA")
  if (!is.null(B)) {
    B <- as.matrix(B); storage.mode(B) <- "double"
    if (nrow(B) != ncol(S)) stop("B must have one row per column of S")
  }
  D <- do.call(cbind, lapply(seq_len(ncol(Y)), function(j) cbind(1, ifelse(is.na(Y[, j]), 0, Y[, j]), B)))
  storage.mode(D) <- "double"
  p <- 2L + (if (is.null(B)) 0L else ncol(B))
  K <- matrix(0, p, 1); K[2, 1] <- 1
  use <- matrix(as.integer(!is.na(Y)), nrow(Y), ncol(Y))
  cn <- if (is.null(colnames(Y))) as.character(seq_len(ncol(Y))) else colnames(Y)
  rn <- if (is.null(rownames(S))) paste0("row", seq_len(nrow(S))) else rownames(S)
  if (length(sort.by) != 1L || !sort.by %in% .limma_sorts) stop("plaid.limma: sort.by must be one of ", paste(.limma_sorts, collapse = ", "))
  weights <- .limma_weights(S, weights)
  .session()
  r <- .limma_call(S, D, ncol(Y), use, K, na, max.na, ncol(Y), rn, sort.by, weights)
  tables <- r$tables
  hyper <- lapply(seq_len(ncol(Y)), function(j) .limma_hyper(r$hyper[, j]))
  names(tables) <- names(hyper) <- cn
  list(tables = tables, hyper = hyper)
}


## the tables of plaid.camera() / plaid.camera.contrasts() from the library's sets x 8 block (NGenes, Correlation, VIF, t,
## Down, Up, PValue, FDR): Direction is "Up" where Up < Down, else "Down" (limma's column), NA on an NA row; ordered by
## sort.by -- "none", "PValue" / "P" / "p" and "FDR" (increasing), "t", "Correlation", "VIF" (decreasing magnitude),
## "NGenes" (decreasing); NA last
.camera_sorts <- c("none", "PValue", "P", "p", "FDR", "t", "Correlation", "VIF", "NGenes")

.camera_table <- function(tab, rn, sort.by) {
  tab <- matrix(tab, nrow = length(rn), ncol = 8L)
  res <- data.frame(NGenes = tab[, 1], Correlation = tab[, 2], VIF = tab[, 3], t = tab[, 4],
                    Direction = ifelse(is.na(tab[, 5]) | is.na(tab[, 6]), NA_character_, ifelse(tab[, 6] < tab[, 5], "Up", "Down")),
                    PValue = tab[, 7], FDR = tab[, 8], row.names = rn, stringsAsFactors = FALSE)
  key <- switch(sort.by, none = NULL, PValue = , P = , p = res$PValue, FDR = res$FDR, t = -abs(res$t),
                Correlation = -abs(res$Correlation), VIF = -abs(res$VIF), NGenes = -res$NGenes,
                stop("plaid.camera: sort.by must be one of ", paste(.camera_sorts, collapse = ", ")))
  if (!is.null(key)) res <- res[order(key), , drop = FALSE]
  res
}

.camera_hyper <- function(h) stats::setNames(as.list(h), c("df.residual", "df.prior", "s2.prior", "n.ok", "n.genes", "df.camera"))

## X as a double matrix with row names, and the sets of G (a gmt list or a genes x sets membership matrix) as the pattern
## (Gp, Gi) over the rows of X: every row of X stays -- camera's universe is all the genes, also those in no set -- and a
## member X does not have is dropped.  Sets outside minSize .. maxSize (default: the genes - 1) members in X are dropped.
.camera_sets <- function(X, G, minSize, maxSize) {
  if (inherits(X, "sparseMatrix")) stop("plaid.camera: X must be dense")
  X <- as.matrix(X); storage.mode(X) <- "double"
  if (is.null(rownames(X))) stop("plaid.camera: X needs row names")
  if (is.list(G)) {
    message("[plaid.camera] converting gmt to sparse matrix...")
    G <- gmt2mat(G)
  }
  G <- methods::as(methods::as(methods::as(G, "dMatrix"), "generalMatrix"), "CsparseMatrix")
  rows <- match(rownames(G), rownames(X))
  rows[duplicated(rownames(G))] <- NA_integer_
  sets <- lapply(seq_len(ncol(G)), function(j) {
    k <- seq.int(G@p[j] + 1L, length.out = G@p[j + 1L] - G@p[j])
    r <- rows[G@i[k] + 1L][G@x[k] != 0]
    sort(r[!is.na(r)]) - 1L
  })
  size <- lengths(sets)
  if (is.null(maxSize)) maxSize <- nrow(X) - 1L
  keep <- which(size >= minSize & size <= maxSize)
  list(X = X, Gp = as.integer(c(0L, cumsum(size[keep]))), Gi = as.integer(unlist(sets[keep])), names = colnames(G)[keep])
}

.camera_call <- function(cs, D, nfit, use, K, inter.gene.cor, allow.neg.cor, ncon, sort.by) {
  rho <- if (is.null(inter.gene.cor) || is.na(inter.gene.cor)) NA_real_ else as.double(inter.gene.cor)
  if (!is.na(rho) && (rho <= -1 || rho >= 1)) stop("plaid.camera: inter.gene.cor must lie inside (-1, 1), or be NA to estimate it")
  if (length(sort.by) != 1L || !sort.by %in% .camera_sorts) stop("plaid.camera: sort.by must be one of ", paste(.camera_sorts, collapse = ", "))
  .session()
  r <- .Call("R_plaidhip_camera", .devices(), cs$X, D, nfit, use, K, cs$Gp, cs$Gi, rho, isTRUE(as.logical(allow.neg.cor)),
             PACKAGE = "plaidhip")
  out <- r[[1]]
  dim(out) <- c(length(cs$names), 8L, ncon)
  list(tables = lapply(seq_len(ncon), function(j) .camera_table(out[, , j], cs$names, sort.by)), hyper = r[[2]], raw = out)
}


## plaid.camera(): limma's competitive gene-set test camera (Wu & Smyth 2012, as pinned in include/plaidhip.h:
## plaidhip_camera) of every set of G on the expression X (genes x samples) for one design (samples x coefficients).
## contrasts, use: as plaid.limma().  The gene statistic is plaid.limma()'s moderated t; a set's two-sample t against the
## other genes is corrected by the variance inflation factor 1 + (m - 1) rho.  inter.gene.cor: the fixed rho (limma's default
## 0.01), or NA / NULL to estimate every set's VIF from the residuals of its genes (allow.neg.cor = FALSE then uses max(VIF, 1)
## in the test; the reported VIF and Correlation stay as estimated).  A gene with an NA in a used sample leaves the universe.
## Returns list(tables = <named list, one data frame per contrast: sets x (NGenes, Correlation, VIF, t, Direction, PValue,
## FDR), ordered by sort.by>, hyper = list(df.residual, df.prior, s2.prior, n.ok, n.genes, df.camera)).
## Not offered: use.ranks, trend.var, weights, a sparse X, na = "fit", fry / roast.
plaid.camera <- function(X, design, G, contrasts = NULL, use = NULL, inter.gene.cor = 0.01, allow.neg.cor = FALSE, minSize = 1,
                         maxSize = NULL, sort.by = "PValue") {
  cs <- .camera_sets(X, G, minSize, maxSize)
  design <- as.matrix(design); storage.mode(design) <- "double"
  if (nrow(design) != ncol(cs$X)) stop("design must have one row per column of X")
  cn <- if (is.null(colnames(design))) paste0("coef", seq_len(ncol(design))) else colnames(design)
  if (!is.null(contrasts)) {
    contrasts <- as.matrix(contrasts); storage.mode(contrasts) <- "double"
    if (nrow(contrasts) != ncol(design)) stop("contrasts must have one row per coefficient")
    cn <- if (is.null(colnames(contrasts))) as.character(seq_len(ncol(contrasts))) else colnames(contrasts)
  }
  if (!is.null(use)) {
    if (length(use) != ncol(cs$X)) stop("use must have one entry per column of X")
    use <- matrix(as.integer(!is.na(use) & use != 0), ncol = 1)
  }
  r <- .camera_call(cs, design, 1L, use, contrasts, inter.gene.cor, allow.neg.cor, length(cn), sort.by)
  tables <- r$tables
  names(tables) <- cn
  list(tables = tables, hyper = .camera_hyper(r$hyper[, 1]))
}


## plaid.camera.contrasts(): plaid.camera() for every column of a contrast matrix Y (samples x contrasts; 0, 1, NA = the
## sample takes no part) in ONE call, with the designs of plaid.limma.contrasts(): contrast j fits [1, Y[, j], B] on the
## samples with a label and tests the sets on the moderated t of the coefficient of Y[, j].  X is uploaded once.  Returns
## list(tables = <named list (the columns of Y) of plaid.camera() tables>, hyper = <named list of their hyper-parameters>).
plaid.camera.contrasts <- function(X, Y, G, B = NULL, inter.gene.cor = 0.01, allow.neg.cor = FALSE, minSize = 1, maxSize = NULL,
                                   sort.by = "PValue") {
  cs <- .camera_sets(X, G, minSize, maxSize)
  Y <- as.matrix(Y)
  if (nrow(Y) != ncol(cs$X)) stop("Y must have one row per column of X")
  if (!all(unique(as.vector(Y)) %in% c(0, 1, NA))) stop("elements of Y must be 0, 1 or NA")
  if (!is.null(B)) {
    B <- as.matrix(B); storage.mode(B) <- "double"
    if (nrow(B) != ncol(cs$X)) stop("B must have one row per column of X")
  }
  D <- do.call(cbind, lapply(seq_len(ncol(Y)), function(j) cbind(1, ifelse(is.na(Y[, j]), 0, Y[, j]), B)))
  storage.mode(D) <- "double"
  p <- 2L + (if (is.null(B)) 0L else ncol(B))
  K <- matrix(0, p, 1); K[2, 1] <- 1
  use <- matrix(as.integer(!is.na(Y)), nrow(Y), ncol(Y))
  cn <- if (is.null(colnames(Y))) as.character(seq_len(ncol(Y))) else colnames(Y)
  r <- .camera_call(cs, D, ncol(Y), use, K, inter.gene.cor, allow.neg.cor, ncol(Y), sort.by)
  tables <- r$tables
  hyper <- lapply(seq_len(ncol(Y)), function(j) .camera_hyper(r$hyper[, j]))
  names(tables) <- names(hyper) <- cn
  list(tables = tables, hyper = hyper)
}


## the tables of plaid.fry() / plaid.fry.contrasts() from the library's sets x 7 block (NGenes, Direction, t, PValue, FDR,
## PValue.Mixed, FDR.Mixed): Direction is "Up" for +1 and "Down" for -1; ordered by sort.by -- "directional" (PValue),
## "mixed" (PValue.Mixed), "none"; NA last
.fry_sorts <- c("directional", "mixed", "none")
.fry_standardize <- c("posterior.sd", "residual.sd", "none")

.fry_table <- function(tab, rn, sort.by) {
  tab <- matrix(tab, nrow = length(rn), ncol = 7L)
  res <- data.frame(NGenes = tab[, 1], Direction = ifelse(is.na(tab[, 2]), NA_character_, ifelse(tab[, 2] > 0, "Up", "Down")),
                    t = tab[, 3], PValue = tab[, 4], FDR = tab[, 5], PValue.Mixed = tab[, 6], FDR.Mixed = tab[, 7],
                    row.names = rn, stringsAsFactors = FALSE)
  key <- switch(sort.by, none = NULL, directional = res$PValue, mixed = res$PValue.Mixed)
  if (!is.null(key)) res <- res[order(key), , drop = FALSE]
  res
}

.fry_hyper <- function(h) stats::setNames(as.list(h), c("df.residual", "df.prior", "s2.prior", "n.ok", "n.genes", "n.effects", "mixed"))

.fry_call <- function(cs, D, nfit, use, K, standardize, ncon, sort.by) {
  if (length(standardize) != 1L || !standardize %in% .fry_standardize)
    stop("plaid.fry: standardize must be one of ", paste(.fry_standardize, collapse = ", "), " (\"p2\" is not offered)")
  if (length(sort.by) != 1L || !sort.by %in% .fry_sorts) stop("plaid.fry: sort.by must be one of ", paste(.fry_sorts, collapse = ", "))
  .session()
  r <- .Call("R_plaidhip_fry", .devices(), cs$X, D, nfit, use, K, cs$Gp, cs$Gi, match(standardize, .fry_standardize) - 1L,
             PACKAGE = "plaidhip")
  out <- r[[1]]
  dim(out) <- c(length(cs$names), 7L, ncon)
  list(tables = lapply(seq_len(ncon), function(j) .fry_table(out[, , j], cs$names, sort.by)), hyper = r[[2]])
}


## plaid.fry(): limma's self-contained rotation gene-set test in closed form (fry: roast with infinitely many rotations, as
## pinned in include/plaidhip.h: plaidhip_fry) of every set of G on the expression X (genes x samples) for one design.  The
## operands are plaid.camera()'s.  camera asks whether a set moves more than the other genes, fry whether the set is
## differential at all; no random number is drawn.  standardize: "posterior.sd" (the default: the effects are plaid.limma()'s
## moderated t), "residual.sd" or "none".  The directional test is complete for any number of samples; the mixed test is
## offered for fits with df.residual + 1 <= 128 effects and NA above that (hyper$mixed = 0).
## Returns list(tables = <named list, one data frame per contrast: sets x (NGenes, Direction, t, PValue, FDR, PValue.Mixed,
## FDR.Mixed), ordered by sort.by>, hyper = list(df.residual, df.prior, s2.prior, n.ok, n.genes, n.effects, mixed)).
## Not offered: roast / mroast, gene or array weights, trend.var, robust, a sparse X, na = "fit", standardize = "p2".
plaid.fry <- function(X, design, G, contrasts = NULL, use = NULL, standardize = "posterior.sd", minSize = 1, maxSize = NULL,
                      sort.by = "directional") {
  cs <- .camera_sets(X, G, minSize, maxSize)
  design <- as.matrix(design); storage.mode(design) <- "double"
  if (nrow(design) != ncol(cs$X)) stop("design must have one row per column of X")
  cn <- if (is.null(colnames(design))) paste0("coef", seq_len(ncol(design))) else colnames(design)
  if (!is.null(contrasts)) {
    contrasts <- as.matrix(contrasts); storage.mode(contrasts) <- "double"
    if (nrow(contrasts) != ncol(design)) stop("contrasts must have one row per coefficient")
    cn <- if (is.null(colnames(contrasts))) as.character(seq_len(ncol(contrasts))) else colnames(contrasts)
  }
  if (!is.null(use)) {
    if (length(use) != ncol(cs$X)) stop("use must have one entry per column of X")
    use <- matrix(as.integer(!is.na(use) & use != 0), ncol = 1)
  }
  r <- .fry_call(cs, design, 1L, use, contrasts, standardize, length(cn), sort.by)
  tables <- r$tables
  names(tables) <- cn
  list(tables = tables, hyper = .fry_hyper(r$hyper[, 1]))
}


## plaid.fry.contrasts(): plaid.fry() for every column of a contrast matrix Y (samples x contrasts; 0, 1, NA = the sample
## takes no part) in ONE call, with the designs of plaid.limma.contrasts().  X is uploaded once.
plaid.fry.contrasts <- function(X, Y, G, B = NULL, standardize = "posterior.sd", minSize = 1, maxSize = NULL,
                                sort.by = "directional") {
  cs <- .camera_sets(X, G, minSize, maxSize)
  Y <- as.matrix(Y)
  if (nrow(Y) != ncol(cs$X)) stop("Y must have one row per column of X")
  if (!all(unique(as.vector(Y)) %in% c(0, 1, NA))) stop("elements of Y must be 0, 1 or NA")
  if (!is.null(B)) {
    B <- as.matrix(B); storage.mode(B) <- "double"
    if (nrow(B) != ncol(cs$X)) stop("B must have one row per column of X")
  }
  D <- do.call(cbind, lapply(seq_len(ncol(Y)), function(j) cbind(1, ifelse(is.na(Y[, j]), 0, Y[, j]), B)))
  storage.mode(D) <- "double"
  p <- 2L + (if (is.null(B)) 0L else ncol(B))
  K <- matrix(0, p, 1); K[2, 1] <- 1
  use <- matrix(as.integer(!is.na(Y)), nrow(Y), ncol(Y))
  cn <- if (is.null(colnames(Y))) as.character(seq_len(ncol(Y))) else colnames(Y)
  r <- .fry_call(cs, D, ncol(Y), use, K, standardize, ncol(Y), sort.by)
  tables <- r$tables
  hyper <- lapply(seq_len(ncol(Y)), function(j) .fry_hyper(r$hyper[, j]))
  names(tables) <- names(hyper) <- cn
  list(tables = tables, hyper = hyper)
}


.roast_statistics <- c("mean", "floormean", "msq", "mean50")
.roast_zscores <- c("hill", "none")
.roast_sorts <- c("directional", "mixed", "none")

.roast_table <- function(tab, rn, sort.by) {
  tab <- matrix(tab, nrow = length(rn), ncol = 8L)
  res <- data.frame(NGenes = tab[, 1], PropDown = tab[, 2], PropUp = tab[, 3],
                    Direction = ifelse(is.na(tab[, 4]), NA_character_, ifelse(tab[, 4] > 0, "Up", "Down")),
                    PValue = tab[, 5], FDR = tab[, 6], PValue.Mixed = tab[, 7], FDR.Mixed = tab[, 8],
                    row.names = rn, stringsAsFactors = FALSE)
  key <- switch(sort.by, none = NULL, directional = res$PValue, mixed = res$PValue.Mixed)
  if (!is.null(key)) res <- res[order(key), , drop = FALSE]
  res
}

.roast_hyper <- function(h) stats::setNames(as.list(h), c("df.residual", "df.prior", "s2.prior", "n.ok", "n.genes", "nrot", "mean50.capped"))

## rotations as the C entry takes them: every fit's (samples + 1) x nrot matrix row by row
.roast_rotations <- function(rotations, n, nfit) {
  if (is.null(rotations)) return(NULL)
  rotations <- if (length(dim(rotations)) == 3L) rotations else array(as.matrix(rotations), c(dim(as.matrix(rotations)), 1L))
  if (dim(rotations)[1] != n + 1L || dim(rotations)[3] != nfit) stop("plaid.roast: rotations must be (samples + 1) x nrot (x fits)")
  storage.mode(rotations) <- "double"
  aperm(rotations, c(2L, 1L, 3L))
}

.roast_call <- function(cs, D, nfit, use, K, set.statistic, nrot, seed, zscore, midp, rotations, ncon, sort.by) {
  if (length(set.statistic) != 1L || !set.statistic %in% .roast_statistics)
    stop("plaid.roast: set.statistic must be one of ", paste(.roast_statistics, collapse = ", "))
  if (length(zscore) != 1L || !zscore %in% .roast_zscores)
    stop("plaid.roast: zscore must be one of ", paste(.roast_zscores, collapse = ", "), " (the exact qnorm(pt()) is not offered)")
  if (length(sort.by) != 1L || !sort.by %in% .roast_sorts) stop("plaid.roast: sort.by must be one of ", paste(.roast_sorts, collapse = ", "))
  rot <- .roast_rotations(rotations, ncol(cs$X), nfit)
  if (!is.null(rot)) nrot <- dim(rot)[1]
  opts <- c(match(set.statistic, .roast_statistics) - 1L, match(zscore, .roast_zscores) - 1L, as.integer(nrot), as.integer(isTRUE(midp)))
  .session()
  r <- .Call("R_plaidhip_roast", .devices(), cs$X, D, nfit, use, K, cs$Gp, cs$Gi, opts, as.double(seed), rot, PACKAGE = "plaidhip")
  out <- r[[1]]
  dim(out) <- c(length(cs$names), 8L, ncon)
  list(tables = lapply(seq_len(ncon), function(j) .roast_table(out[, , j], cs$names, sort.by)), hyper = r[[2]])
}


## plaid.roast(): limma's rotation gene-set test with sampled rotations (roast / mroast as pinned in include/plaidhip.h:
## plaidhip_roast) of every set of G on the expression X (genes x samples) for one design.  The operands are plaid.fry()'s.
## What it adds to plaid.fry(): a mixed test for any number of samples, and the set statistics "mean50" (the default),
## "floormean" and "msq" beside "mean".  The rotations are drawn in sample space from `seed` and shared by every set and
## contrast (as romer shares them; mroast draws per set), or given: rotations, (samples + 1) x nrot with row 1 = r0.
## p = (b + 1) / (nrot + 1); midp takes the FDR on p - 0.5 / (nrot + 1).  Under "mean50" a set with more than 16,384 members
## in the universe has NA p-values (hyper$mean50.capped = 1).
## Returns list(tables = <named list, one data frame per contrast: sets x (NGenes, PropDown, PropUp, Direction, PValue, FDR,
## PValue.Mixed, FDR.Mixed), ordered by sort.by>, hyper = list(df.residual, df.prior, s2.prior, n.ok, n.genes, nrot,
## mean50.capped)).
## Not offered: per-set rotations, gene or array weights, trend.var, robust, a sparse X, na = "fit", the exact z-score; romer is
## plaid.romer(), below.
plaid.roast <- function(X, design, G, contrasts = NULL, use = NULL, set.statistic = "mean50", nrot = 1999, seed = 1,
                        zscore = "hill", midp = TRUE, rotations = NULL, minSize = 1, maxSize = NULL, sort.by = "directional") {
  cs <- .camera_sets(X, G, minSize, maxSize)
  design <- as.matrix(design); storage.mode(design) <- "double"
  if (nrow(design) != ncol(cs$X)) stop("design must have one row per column of X")
  cn <- if (is.null(colnames(design))) paste0("coef", seq_len(ncol(design))) else colnames(design)
  if (!is.null(contrasts)) {
    contrasts <- as.matrix(contrasts); storage.mode(contrasts) <- "double"
    if (nrow(contrasts) != ncol(design)) stop("contrasts must have one row per coefficient")
    cn <- if (is.null(colnames(contrasts))) as.character(seq_len(ncol(contrasts))) else colnames(contrasts)
  }
  if (!is.null(use)) {
    if (length(use) != ncol(cs$X)) stop("use must have one entry per column of X")
    use <- matrix(as.integer(!is.na(use) & use != 0), ncol = 1)
  }
  r <- .roast_call(cs, design, 1L, use, contrasts, set.statistic, nrot, seed, zscore, midp, rotations, length(cn), sort.by)
  tables <- r$tables
  names(tables) <- cn
  list(tables = tables, hyper = .roast_hyper(r$hyper[, 1]))
}


## plaid.roast.contrasts(): plaid.roast() for every column of a contrast matrix Y (samples x contrasts; 0, 1, NA = the sample
## takes no part) in ONE call, with the designs of plaid.limma.contrasts().  X is uploaded once.  Contrast j is fit number j:
## its generated rotations are those of (seed, j - 1).
plaid.roast.contrasts <- function(X, Y, G, B = NULL, set.statistic = "mean50", nrot = 1999, seed = 1, zscore = "hill",
                                  midp = TRUE, rotations = NULL, minSize = 1, maxSize = NULL, sort.by = "directional") {
  cs <- .camera_sets(X, G, minSize, maxSize)
  Y <- as.matrix(Y)
  if (nrow(Y) != ncol(cs$X)) stop("Y must have one row per column of X")
  if (!all(unique(as.vector(Y)) %in% c(0, 1, NA))) stop("elements of Y must be 0, 1 or NA")
  if (!is.null(B)) {
    B <- as.matrix(B); storage.mode(B) <- "double"
    if (nrow(B) != ncol(cs$X)) stop("B must have one row per column of X")
  }
  D <- do.call(cbind, lapply(seq_len(ncol(Y)), function(j) cbind(1, ifelse(is.na(Y[, j]), 0, Y[, j]), B)))
  storage.mode(D) <- "double"
  p <- 2L + (if (is.null(B)) 0L else ncol(B))
  K <- matrix(0, p, 1); K[2, 1] <- 1
  use <- matrix(as.integer(!is.na(Y)), nrow(Y), ncol(Y))
  cn <- if (is.null(colnames(Y))) as.character(seq_len(ncol(Y))) else colnames(Y)
  r <- .roast_call(cs, D, ncol(Y), use, K, set.statistic, nrot, seed, zscore, midp, rotations, ncol(Y), sort.by)
  tables <- r$tables
  hyper <- lapply(seq_len(ncol(Y)), function(j) .roast_hyper(r$hyper[, j]))
  names(tables) <- names(hyper) <- cn
  list(tables = tables, hyper = hyper)
}


.romer_statistics <- c("mean", "floormean", "mean50")
.romer_sorts <- c("none", "up", "down", "mixed")

.romer_table <- function(tab, rn, sort.by) {
  tab <- matrix(tab, nrow = length(rn), ncol = 7L)
  res <- data.frame(NGenes = tab[, 1], Up = tab[, 2], Down = tab[, 3], Mixed = tab[, 4], FDR.Up = tab[, 5], FDR.Down = tab[, 6],
                    FDR.Mixed = tab[, 7], row.names = rn, stringsAsFactors = FALSE)
  key <- switch(sort.by, none = NULL, up = res$Up, down = res$Down, mixed = res$Mixed)
  if (!is.null(key)) res <- res[order(key), , drop = FALSE]
  res
}

.romer_hyper <- function(h, cn) {
  c(stats::setNames(as.list(h[1:8]), c("df.residual", "df.prior", "s2.prior", "n.ok", "n.genes", "nrot", "mean50.capped", "nan.t")),
    list(proportion = stats::setNames(h[-(1:8)], cn)))
}

.romer_call <- function(cs, D, nfit, use, K, set.statistic, nrot, seed, shrink.resid, rotations, ncon, sort.by) {
  if (length(set.statistic) != 1L || !set.statistic %in% .romer_statistics)
    stop("plaid.romer: set.statistic must be one of ", paste(.romer_statistics, collapse = ", "))
  if (length(sort.by) != 1L || !sort.by %in% .romer_sorts) stop("plaid.romer: sort.by must be one of ", paste(.romer_sorts, collapse = ", "))
  rot <- .roast_rotations(rotations, ncol(cs$X), nfit)
  if (!is.null(rot)) nrot <- dim(rot)[1]
  opts <- c(match(set.statistic, .romer_statistics) - 1L, as.integer(nrot), as.integer(isTRUE(shrink.resid)))
  .session()
  r <- .Call("R_plaidhip_romer", .devices(), cs$X, D, nfit, use, K, cs$Gp, cs$Gi, opts, as.double(seed), rot, PACKAGE = "plaidhip")
  out <- r[[1]]
  dim(out) <- c(length(cs$names), 7L, ncon)
  list(tables = lapply(seq_len(ncon), function(j) .romer_table(out[, , j], cs$names, sort.by)), hyper = r[[2]])
}


## plaid.romer(): limma's rotation GSEA (romer as pinned in include/plaidhip.h: plaidhip_romer) of every set of G on the
## expression X (genes x samples) for one design.  The operands are plaid.roast()'s.  It is the COMPETITIVE test with a rotation
## null: under every rotation the genes' moderated t are ranked among all genes and a set takes the sum of its members' ranks, so
## the null keeps the gene-gene correlation.  set.statistic: "mean" (the default), "floormean" or "mean50".  shrink.resid
## (limma's default) shrinks the observed effects by the empirical-Bayes posterior before rotating.  The rotations are
## plaid.roast()'s, drawn in sample space from `seed` and shared by every set and contrast, or given: rotations, (samples + 1)
## x nrot with row 1 = r0.  p = (b + 1) / (nrot + 1) from exact integer statistics.  Under "mean50" a set with more than 16,384
## members in the universe has NA p-values (hyper$mean50.capped = 1).
## Returns list(tables = <named list, one data frame per contrast: sets x (NGenes, Up, Down, Mixed, FDR.Up, FDR.Down,
## FDR.Mixed), ordered by sort.by>, hyper = list(df.residual, df.prior, s2.prior, n.ok, n.genes, nrot, mean50.capped, nan.t,
## proportion)).
## Not offered: array.weights, block / correlation, a sparse X, na = "fit", gene weights, trend, robust.
plaid.romer <- function(X, design, G, contrasts = NULL, use = NULL, set.statistic = "mean", nrot = 9999, seed = 1,
                        shrink.resid = TRUE, rotations = NULL, minSize = 1, maxSize = NULL, sort.by = "none") {
  cs <- .camera_sets(X, G, minSize, maxSize)
  design <- as.matrix(design); storage.mode(design) <- "double"
  if (nrow(design) != ncol(cs$X)) stop("design must have one row per column of X")
  cn <- if (is.null(colnames(design))) paste0("coef", seq_len(ncol(design))) else colnames(design)
  if (!is.null(contrasts)) {
    contrasts <- as.matrix(contrasts); storage.mode(contrasts) <- "double"
    if (nrow(contrasts) != ncol(design)) stop("contrasts must have one row per coefficient")
    cn <- if (is.null(colnames(contrasts))) as.character(seq_len(ncol(contrasts))) else colnames(contrasts)
  }
  if (!is.null(use)) {
    if (length(use) != ncol(cs$X)) stop("use must have one entry per column of X")
    use <- matrix(as.integer(!is.na(use) & use != 0), ncol = 1)
  }
  r <- .romer_call(cs, design, 1L, use, contrasts, set.statistic, nrot, seed, shrink.resid, rotations, length(cn), sort.by)
  tables <- r$tables
  names(tables) <- cn
  list(tables = tables, hyper = .romer_hyper(r$hyper[, 1], cn))
}


## plaid.romer.contrasts(): plaid.romer() for every column of a contrast matrix Y (samples x contrasts; 0, 1, NA = the sample
## takes no part) in ONE call, with the designs of plaid.limma.contrasts().  X is uploaded once.  Contrast j is fit number j:
## its generated rotations are those of (seed, j - 1).
plaid.romer.contrasts <- function(X, Y, G, B = NULL, set.statistic = "mean", nrot = 9999, seed = 1, shrink.resid = TRUE,
                                  rotations = NULL, minSize = 1, maxSize = NULL, sort.by = "none") {
  cs <- .camera_sets(X, G, minSize, maxSize)
  Y <- as.matrix(Y)
  if (nrow(Y) != ncol(cs$X)) stop("Y must have one row per column of X")
  if (!all(unique(as.vector(Y)) %in% c(0, 1, NA))) stop("elements of Y must be 0, 1 or NA")
  if (!is.null(B)) {
    B <- as.matrix(B); storage.mode(B) <- "double"
    if (nrow(B) != ncol(cs$X)) stop("B must have one row per column of X")
  }
  D <- do.call(cbind, lapply(seq_len(ncol(Y)), function(j) cbind(1, ifelse(is.na(Y[, j]), 0, Y[, j]), B)))
  storage.mode(D) <- "double"
  p <- 2L + (if (is.null(B)) 0L else ncol(B))
  K <- matrix(0, p, 1); K[2, 1] <- 1
  use <- matrix(as.integer(!is.na(Y)), nrow(Y), ncol(Y))
  cn <- if (is.null(colnames(Y))) as.character(seq_len(ncol(Y))) else colnames(Y)
  r <- .romer_call(cs, D, ncol(Y), use, K, set.statistic, nrot, seed, shrink.resid, rotations, ncol(Y), sort.by)
  tables <- r$tables
  hyper <- lapply(seq_len(ncol(Y)), function(j) .romer_hyper(r$hyper[, j], cn[j]))
  names(tables) <- names(hyper) <- cn
  list(tables = tables, hyper = hyper)
}


## plaid.intergenecor(): limma's interGeneCorrelation(X[set, ], design) for every set of G at once: the variance inflation
## factor of the set's mean, estimated from the residuals of its genes, and the mean pairwise correlation (VIF - 1) / (m - 1).
## Returns a matrix, sets x (NGenes, Correlation, VIF), in G's order.
plaid.intergenecor <- function(X, design, G, use = NULL, minSize = 1, maxSize = NULL) {
  cs <- .camera_sets(X, G, minSize, maxSize)
  design <- as.matrix(design); storage.mode(design) <- "double"
  if (nrow(design) != ncol(cs$X)) stop("design must have one row per column of X")
  if (!is.null(use)) {
    if (length(use) != ncol(cs$X)) stop("use must have one entry per column of X")
    use <- matrix(as.integer(!is.na(use) & use != 0), ncol = 1)
  }
  K <- matrix(0, ncol(design), 1); K[1, 1] <- 1   # (any contrast: the VIF does not depend on it)
  r <- .camera_call(cs, design, 1L, use, K, NA_real_, TRUE, 1L, "none")
  matrix(r$raw[, 1:3, 1], nrow = length(cs$names), dimnames = list(cs$names, c("NGenes", "Correlation", "VIF")))
}


## replaid.gsva(), R/plaid.R:338-363: the row transform ("z" or "ecdf"), the signed ranks, the power and
## plaid() run on the device in one call.
replaid.gsva <- function(X, matG, tau = 0, rowtf = c("z", "ecdf")[1]) {
  rowtf <- rowtf[1]
  if (!rowtf %in% c("z", "ecdf")) stop("Error: unknown row transform", rowtf)
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  .session()
  dev <- .devices()
  if (length(dev) > 1L && rowtf != "ecdf") {
    ## sample shards over several GPUs (the per-gene mean and sd are combined across them); "ecdf" needs every
    ## sample of a gene on one device and takes the single-device route below
    if (methods::is(X, "sparseMatrix")) X <- methods::as(X, "generalMatrix")
    xa <- .x_args(X)
    S <- .Call("R_plaidhip_gsva_multi", dev, xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi, as.numeric(tau),
               0L, PACKAGE = "plaidhip")
  } else if (inherits(X, "CsparseMatrix")) {
    ## the row statistics are taken from the CSC slots on the device (a row view built there): X stays sparse
    X <- methods::as(X, "generalMatrix")
    S <- .Call("R_plaidhip_gsva_csc", X@p, X@i, as.double(X@x), nrow(X), pat$Gp, pat$Gi, as.numeric(tau),
               as.integer(rowtf == "ecdf"), PACKAGE = "plaidhip")
  } else {
    D <- as.matrix(X); storage.mode(D) <- "double"
    S <- .Call("R_plaidhip_gsva", D, pat$Gp, pat$Gi, as.numeric(tau), as.integer(rowtf == "ecdf"), PACKAGE = "plaidhip")
  }
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

## The random-walk statistic of GSVA (Haenzelmann et al. 2013) -- replaid.gsva is the reference's approximation, a mean
## of transformed ranks (R/plaid.R:353-356).  include/plaidhip.h (plaidhip_gsva_exact) pins it: the row transform v of X
## ("z" and "ecdf" as replaid.gsva's, "none": X as it is, for a caller's own per-gene CDF, "gauss": GSVA's default, the
## Gaussian kernel CDF estimate of every value among its gene's samples with bandwidth sd / 4, as the sum over the samples
## without GSVA's division by n and its logit, which keep a sample's order; at least 2 samples); per sample the genes in
## order(v, decreasing = TRUE), ties in row order; the gene at position pos weighs abs((N + 1 - pos) - N / 2)^tau; a
## Kolmogorov-Smirnov walk per set whose largest positive and largest negative excursion are added (max.diff = TRUE) or
## the larger of which is returned (FALSE; the negative one when equal).  Sets without aligned members, with all genes,
## or of zero total weight score NA; a sample holding an NA scores NA for every set.  Differs from GSVA::gsva on purpose:
## the running sum is evaluated at the hits (three roundings per value, where GSVA's loop accumulates N), a set of zero
## total weight is NA, and abs.ranking and the Poisson kernel (kcdf = "Poisson") are not offered.  No normalize_medians.
## nrow(X) at most 131,072.  options(plaidhip.devices = ...) shards the samples; "ecdf" takes one device, "gauss" sends all
## of X to every device.
replaid.gsva.exact <- function(X, matG, tau = 1, rowtf = c("z", "ecdf", "none", "gauss")[1], max.diff = TRUE) {
  rowtf <- rowtf[1]
  if (!rowtf %in% c("z", "ecdf", "none", "gauss")) stop("Error: unknown row transform", rowtf)
  if (rowtf == "gauss" && ncol(X) < 2L) stop("gsva_exact: rowtf = \"gauss\" needs at least 2 samples")
  tau <- as.double(tau)
  if (length(tau) != 1L || !is.finite(tau) || tau < 0) stop("gsva_exact: tau must be finite and >= 0")
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  .session()
  if (methods::is(X, "sparseMatrix")) X <- methods::as(X, "generalMatrix")
  xa <- .x_args(X)
  tf <- match(rowtf, c("z", "ecdf", "none", "gauss")) - 1L
  dev <- .devices()
  S <- if (length(dev) > 1L && rowtf != "ecdf")
         .Call("R_plaidhip_gsva_exact_multi", dev, xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi, tau, tf,
               isTRUE(as.logical(max.diff)), PACKAGE = "plaidhip")
       else .Call("R_plaidhip_gsva_exact", xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi, tau, tf,
                  isTRUE(as.logical(max.diff)), PACKAGE = "plaidhip")
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

## GSVA's method = "plage" (Tomfohr et al. 2005), the third of the four methods of the reference's gset.gsva
## (experiments/R/functions.R:148-160): per set the first right singular vector of the standardized expression block of its
## genes -- svd(Z_s)$v[, 1], the set's "activity" across the samples.  include/plaidhip.h (plaidhip_plage) pins it: genes
## standardized over all samples as scale() does (no 1e-8), constant genes left out of every set, a gene holding NA / Inf
## making its sets NA; the eigenvector by power iteration from the largest column of Z_s Z_s' (tol, maxit: its stop test and
## step cap).  The sign, arbitrary in LAPACK and so in GSVA, is pinned: the score rises when the set's genes rise on average
## (a balanced pair: its first gene is positive).  Sets with fewer than minSize or more than maxSize aligned members are
## dropped; sets above 4,096 members are not offered.  Returns the sets x samples scores with attribute "info": sets x (size,
## lambda, explained, iterations, residual, converged); loadings = TRUE adds attribute "loadings", a named list of the sets'
## loadings over their aligned genes (0 for a dropped constant gene).  options(plaidhip.devices = ...) shards the samples;
## every device takes all of X.
replaid.plage <- function(X, matG, minSize = 1, maxSize = NULL, tol = 2^-40, maxit = 1000L, loadings = FALSE) {
  if (!is.null(maxSize) && maxSize > 4096L) stop("replaid.plage: maxSize = ", maxSize, " (at most 4096 members)")
  tol <- as.double(tol)
  if (length(tol) != 1L || is.na(tol) || tol <= 0) stop("replaid.plage: tol = ", tol, " (a positive number)")
  maxit <- as.integer(maxit)
  if (length(maxit) != 1L || is.na(maxit) || maxit < 1L) stop("replaid.plage: maxit = ", maxit, " (at least 1)")
  if (ncol(X) < 2L) stop("plage: ", ncol(X), " samples (at least 2)")
  gg <- intersect(rownames(matG), rownames(X))
  if (length(gg) == 0L) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  size <- Matrix::colSums(matG[gg, , drop = FALSE] != 0)
  keep <- size >= minSize & (if (is.null(maxSize)) TRUE else size <= maxSize)
  if (any(size[keep] > 4096L)) stop("replaid.plage: a set of ", max(size[keep]), " members (at most 4096; set maxSize)")
  matG <- matG[, keep, drop = FALSE]
  pat <- .aligned_pattern(X, matG)
  .session()
  if (methods::is(X, "sparseMatrix")) X <- methods::as(X, "generalMatrix")
  xa <- .x_args(X)
  r <- .Call("R_plaidhip_plage", .devices(), xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi, tol, maxit,
             isTRUE(as.logical(loadings)), PACKAGE = "plaidhip")
  S <- r[[1]]
  dimnames(S) <- list(colnames(matG), colnames(X))
  info <- r[[2]]
  dimnames(info) <- list(colnames(matG), c("size", "lambda", "explained", "iterations", "residual", "converged"))
  attr(S, "info") <- info
  if (isTRUE(as.logical(loadings))) {
    L <- lapply(seq_len(ncol(matG)), function(j) {
      seg <- seq_len(pat$Gp[j + 1L] - pat$Gp[j]) + pat$Gp[j]
      stats::setNames(r[[3]][seg], rownames(X)[pat$Gi[seg] + 1L])
    })
    names(L) <- colnames(matG)
    attr(S, "loadings") <- L
  }
  S
}

## GSVA's method = "zscore" (Lee et al. 2008), the fourth: the sum of a set's standardized genes over the square root of
## their number.  include/plaidhip.h (plaidhip_zscore) pins it: the standardization of replaid.plage; a set without a kept
## gene scores NA, and so does every set holding a gene with NA / Inf.  Returns sets x samples.
## options(plaidhip.devices = ...) shards the samples; every device takes all of X.
replaid.zscore <- function(X, matG) {
  if (ncol(X) < 2L) stop("zscore: ", ncol(X), " samples (at least 2)")
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  .session()
  if (methods::is(X, "sparseMatrix")) X <- methods::as(X, "generalMatrix")
  xa <- .x_args(X)
  S <- .Call("R_plaidhip_zscore", .devices(), xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X), pat$Gp, pat$Gi, PACKAGE = "plaidhip")
  dimnames(S) <- list(colnames(matG), colnames(X))
  S
}

## singscore's normalised score and dispersion -- replaid.sing (R/plaid.R:213-219) returns mean(rank) / N - 0.5, which
## orders the samples as singscore does and nothing more.  The formulas follow singscore's rankGenes and singscoring AS
## RECALLED (the package's source is not in this tree); include/plaidhip.h (plaidhip_sing_exact) pins them: per sample
## r = rank(x, ties = "min") over ALL rows of X; for a set with k aligned members of ranks s the score is
## (mean(s) - (k + 1) / 2) / (N - k), minus 0.5 when center; the dispersion is mad(s) = 1.4826 * median(|s - median(s)|).
## matD (optional): the down sets, column j pairing with column j of matG, scored on N + 1 - r; Total = Up + Down.  Sets
## without aligned members or with all N genes score NA (the dispersion of all N genes is finite); an empty down column
## makes its Total NA; a sample holding an NA is NA everywhere.  Returns a list of sets x samples matrices: UpScore,
## UpDispersion and, with matD, TotalScore, DownScore, TotalDispersion, DownDispersion.  dispersion = FALSE returns the
## scores alone and runs no per-pair kernel.  With the dispersion nrow(X) is at most 131,072.  Not offered:
## knownDirection = FALSE, other dispersion functions, stable genes, permutation p-values.
## options(plaidhip.devices = ...) shards the samples.
replaid.sing.exact <- function(X, matG, matD = NULL, center = TRUE, dispersion = TRUE) {
  if (!is.null(matD) && ncol(matD) != ncol(matG)) stop("sing_exact: matD has ", ncol(matD), " columns, matG ", ncol(matG))
  pat <- .aligned_pattern(X, matG)
  if (is.null(pat)) { message("[plaid] ERROR. No overlapping features."); return(NULL) }
  Dp <- integer(0); Di <- integer(0)
  if (!is.null(matD)) {
    dpat <- .aligned_pattern(X, matD)
    if (is.null(dpat)) dpat <- list(Gp = integer(ncol(matD) + 1L), Gi = integer(0))
    Dp <- dpat$Gp; Di <- dpat$Gi
  }
  .session()
  if (methods::is(X, "sparseMatrix")) X <- methods::as(X, "generalMatrix")
  xa <- .x_args(X)
  dev <- .devices()
  res <- .Call("R_plaidhip_sing_exact", if (length(dev) > 1L) dev else integer(0), xa[[1]], xa[[2]], xa[[3]], nrow(X), ncol(X),
               pat$Gp, pat$Gi, Dp, Di, isTRUE(as.logical(center)), isTRUE(as.logical(dispersion)), PACKAGE = "plaidhip")
  names(res) <- c("TotalScore", "UpScore", "DownScore", "TotalDispersion", "UpDispersion", "DownDispersion")
  res <- res[!vapply(res, is.null, logical(1))]
  lapply(res, function(S) { dimnames(S) <- list(colnames(matG), colnames(X)); S })
}
