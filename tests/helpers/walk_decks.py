"""Decks of sets for the task loops of the bitmap-walk kernels (host only: numpy and the host restatements).

Every exact walk keeps an N-bit map in LDS that is all zero on the way into a (set, column) pair and has to be on the way
out (plaid_amd/csrc/bitmap_walk.h), and its kernels loop over tasks on a capped grid: once a launch has more tasks than
the cap, workgroup w takes the tasks w, w + grid, w + 2 grid, ... and hands its map (gsea_null_kernel: its s_es area as
well) from one to the next.  Here a task is a set -- eight columns or lists at most, so there is one column tile or list
tile -- and a deck of m = stride + tail sets, each a copy of one of K distinct member lists ("kinds"), is dealt with
tests/helpers/rank_decks.py so that every kind follows every kind (itself included) inside some workgroup or wavefront.
The reference is computed on the K distinct lists and expanded by index (`expand`): K x columns host walks, whatever m.

The strides restate the launch functions; tests/test_walk_decks_host.py holds the decks to their conditions for 64, 256
and 304 CUs, tests/test_gpu_walk_tasks.py for the device it runs on.

N = 4,160 genes: two scan steps of the map (4,096 positions and 64 more), and an even N, which has the centre gene
(q = N / 2) whose weight |q - N / 2|^tau is 0 in replaid.gsva.exact."""
import numpy as np

from . import rank_decks as rd

N = 4160
STEP = 4096                   # positions of one scan step: 64 words of 64 bits
NCOL = 8                      # columns of X: one column tile (kKsColTile = kMadColTile = 16), four wavefronts, two columns each
NAN_COLS = (0, 5)             # wavefront 0 meets column 0 (NaN) and then column 4; wavefront 1 column 1 and then column 5 (NaN)
LIST_TILE = 8                 # kGnListTile (kernels_gsea.hip)
PERM_BLOCK = 64               # kGnBlock

# (`both` first: rank_decks.deck gives every workgroup that has one task only the first kind of its cycle)
KS_KINDS = ("both", "empty", "full", "one", "k64", "k65", "high", "low", "centre")
GSEA_KINDS = ("both", "empty", "full", "one", "k64", "k65", "high", "low", "zero_w")
NAN_KINDS = ("empty", "full")             # k = 0 and k = N: NaN for every walk, the map untouched


# ---- the strides: tasks (pairs) between two tasks of one workgroup (wavefront) once the grid is capped -------------------------
def ks_stride(cu):
    """ks_launch (kernels_ks.hip) and launch_sing_mad (kernels_sing.hip): at most 32 x CUs workgroups, a task each"""
    return 32 * cu


def pair_stride(cu):
    """gn_pair_launch (kernels_gsea.hip; gsea_obs_kernel, gsea_edge_kernel): at most 16 x CUs workgroups of kGnWaves = 4
    wavefronts, a (set, list) pair per wavefront"""
    return 16 * cu * 4


def null_stride(cu):
    """launch_gsea_null (kernels_gsea.hip): at most 16 x CUs workgroups, a task each"""
    return 16 * cu


# ---- the genes -------------------------------------------------------------------------------------------------------------------
def gene_groups(seed=1):
    """rows of the deck's genes: `high` (the 64 largest values of every column), `low` (the 64 smallest), `centre` (the gene
    with last rank N / 2 in every column), `zero` (20 genes that weigh 0 in every list of a weighted plaid.gsea call), `one`
    (the member of the one-gene kind) and `middle` (every other row, `zero` and `one` included)"""
    p = np.random.default_rng(seed).permutation(N)
    return {"high": np.sort(p[:64]), "low": np.sort(p[64:128]), "centre": int(p[128]), "zero": np.sort(p[129:149]),
            "one": int(p[149]), "middle": np.sort(p[129:])}


def _tied_values(q):
    """values with the order of the ranks q (1..N): the 64 smallest, the 64 largest and rank N / 2 stay alone, the ranks
    between them tie in threes -- inside a tie the last ranks differ from q, the ranks a group holds do not"""
    x = q.astype(np.float64)
    half = N // 2
    for lo, hi in ((65, half - 1), (half + 1, N - 64)):
        sel = (q >= lo) & (q <= hi)
        x[sel] = lo + 3 * ((q[sel] - lo) // 3)
    return x


def columns(ncol=NCOL, nan_cols=NAN_COLS, seed=2):
    """X (N x ncol, Fortran order) of integers with ties.  In every column the rows `high` hold the 64 largest values, the
    rows `low` the 64 smallest and the row `centre` last rank N / 2: so `high` stands at the walk positions 0..63 (the first
    scan step) of the ks kernels and plaid.gsea's observed placement (bit N - q) and at the bits 4,096..4,159 (the second)
    of sing_mad_kernel (bit q - 1), `low` the other way round.  A column in nan_cols holds one NaN."""
    rng = np.random.default_rng(seed)
    gg = gene_groups()
    X = np.empty((N, ncol), order="F")
    for c in range(ncol):
        q = np.empty(N, dtype=np.int64)
        q[gg["high"]] = N - 63 + rng.permutation(64)
        q[gg["low"]] = 1 + rng.permutation(64)
        q[gg["centre"]] = N // 2
        rest = np.setdiff1d(np.arange(65, N - 63), [N // 2])
        q[gg["middle"]] = rng.permutation(rest)
        X[:, c] = _tied_values(q)
    for c in nan_cols:
        X[(37 * (c + 1)) % N, c] = np.nan
    return X


def gsea_weights(ncol, weighted, seed=3):
    """weights of a plaid.gsea call (N x ncol): 1, or integers below 2^20 of which the rows `zero` and about a quarter of the
    others weigh 0 in every list (the row `one` never does): the kind zero_w has B = 0 under the observed placement, and
    the one-gene kind under about a quarter of the null placements"""
    if not weighted:
        return np.ones((N, ncol))
    rng = np.random.default_rng(seed)
    gg = gene_groups()
    w = rng.integers(1, 2**20, size=(N, ncol)).astype(np.float64)
    w[rng.random(size=(N, ncol)) < 0.25] = 0.0
    w[gg["one"], :] = rng.integers(1, 2**20, size=ncol)
    w[gg["zero"], :] = 0.0
    return w


def placements(B, seed=4):
    """N x B int32 placements (Fortran order), random permutations"""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.stack([rng.permutation(N) for _ in range(B)], axis=1).astype(np.int32))


# ---- the kinds -------------------------------------------------------------------------------------------------------------------
def member_lists(kinds, seed=5):
    """{kind: sorted int32 rows}"""
    rng = np.random.default_rng(seed)
    gg = gene_groups()
    plain = np.setdiff1d(gg["middle"], np.concatenate([gg["zero"], [gg["one"]]]))
    every = {
        "empty": np.empty(0, dtype=np.int64),
        "full": np.arange(N),
        "one": np.array([gg["one"]]),
        "k64": rng.choice(N, size=64, replace=False),
        "k65": rng.choice(N, size=65, replace=False),
        "high": rng.choice(gg["high"], size=40, replace=False),
        "low": rng.choice(gg["low"], size=40, replace=False),
        "both": np.concatenate([rng.choice(gg["high"], size=20, replace=False), rng.choice(gg["low"], size=20, replace=False),
                                rng.choice(plain, size=100, replace=False)]),
        "centre": np.array([gg["centre"]]),
        "zero_w": gg["zero"],
    }
    return {k: np.sort(every[k]).astype(np.int32) for k in kinds}


def pattern_of(lists_in_order):
    lens = [len(r) for r in lists_in_order]
    Gp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    Gi = np.concatenate(lists_in_order).astype(np.int32) if lens else np.empty(0, dtype=np.int32)
    return Gp, Gi


def kinds_pattern(kinds):
    """(Gp, Gi) of the K distinct lists, in the order of `kinds`: what the reference is computed on"""
    ml = member_lists(kinds)
    return pattern_of([ml[k] for k in kinds])


def deal(kinds, stride, extra=7):
    """the kind of each of stride + K^2 + extra sets: every ordered pair of kinds inside some workgroup on a grid of
    `stride` (rank_decks.deck raises where a launch is too short for that).  Returns (names, idx): idx the kind's index"""
    kinds = tuple(kinds)
    names = rd.deck(kinds, stride, 1, len(kinds) ** 2 + extra)
    if rd.pairs_seen(names, stride) != rd.all_pairs(kinds):
        raise ValueError(f"the deck of {len(names)} sets shows not every ordered pair of {len(kinds)} kinds at stride {stride}")
    return names, np.array([kinds.index(k) for k in names])


def deck_pattern(kinds, idx):
    """(Gp, Gi) of the deck: set j is a copy of the list of kind idx[j]"""
    ml = member_lists(kinds)
    return pattern_of([ml[kinds[i]] for i in idx])


def expand(rows, idx):
    """a reference computed on the K distinct lists (first axis K), set by set of the deck"""
    return np.asarray(rows)[np.asarray(idx)]


def expand_segments(le_idx, Gp_kinds, idx):
    """the edge buffer (nnz of the K lists x lists) of gsea_edge_ref, segment by segment of the deck"""
    segs = [le_idx[Gp_kinds[i]:Gp_kinds[i + 1]] for i in range(len(Gp_kinds) - 1)]
    return np.asfortranarray(np.concatenate([segs[i] for i in idx], axis=0))


def copies_differ(out, idx):
    """sets whose row of `out` (first axis: sets) has not the bits of the first copy of its kind"""
    out = np.ascontiguousarray(out)
    flat = out.reshape(out.shape[0], -1)
    first = np.full(int(np.max(idx)) + 1, -1, dtype=np.int64)
    for j in range(len(idx) - 1, -1, -1):
        first[idx[j]] = j
    model = flat[first[idx]]
    if flat.dtype == np.float64:
        same = (flat.view(np.int64) == model.view(np.int64)) | (np.isnan(flat) & np.isnan(model))
    else:
        same = flat == model
    return np.flatnonzero(~np.all(same, axis=1))


def nan_only_where(rows, kinds, nan_kinds, nan_cols):
    """whether a reference on the K lists (K x columns) is NaN for the kinds nan_kinds and in the columns nan_cols, and
    finite everywhere else"""
    rows = np.asarray(rows)
    want = np.zeros(rows.shape, dtype=bool)
    want[[i for i, k in enumerate(kinds) if k in nan_kinds], :] = True
    want[:, list(nan_cols)] = True
    return bool(np.array_equal(np.isnan(rows), want) and np.isfinite(rows[~want]).all())


# ---- what stands where -----------------------------------------------------------------------------------------------------------
def bits_of(X, rows, entry):
    """the map bits of the rows in every NaN-free column: N - q for the ks kernels and plaid.gsea's observed placement
    ("ks"), q - 1 for sing_mad_kernel ("mad"), q the last ranks"""
    from .ssgsea_walk import last_ranks
    ok = ~np.isnan(X).any(axis=0)
    q = last_ranks(X[:, ok]).astype(np.int64)[np.asarray(rows, dtype=np.int64)]
    return N - q if entry == "ks" else q - 1


# ---- gsea_null_kernel's task order -----------------------------------------------------------------------------------------------
def null_tasks(m, c, B, weighted=True):
    """(blk, tile, j, nb, nl) of every task of one gsea_null_kernel launch over B placements, in task order
    (task = blk * m * ntile + tile * m + j): nb placements in the block, nl lists in the tile"""
    ntile = (c + LIST_TILE - 1) // LIST_TILE if weighted else 1
    nblk = (B + PERM_BLOCK - 1) // PERM_BLOCK
    t = np.arange(m * ntile * nblk, dtype=np.int64)
    blk, rem = t // (m * ntile), t % (m * ntile)
    tile, j = rem // m, rem % m
    nb = np.minimum(PERM_BLOCK, B - blk * PERM_BLOCK)
    nl = np.minimum(LIST_TILE, c - tile * LIST_TILE) if weighted else np.full(len(t), c)
    return blk, tile, j, nb, nl


def null_successions(names, c, B, grid, weighted=True):
    """what the workgroups of a capped launch meet: {"block": a full block of placements followed by the partial one,
    "tile": the full list tile followed by the short one, "from_nan": one of those whose first task is a set of a
    NaN-scoring kind}, each a count of successions task -> task + grid"""
    m = len(names)
    blk, tile, j, nb, nl = null_tasks(m, c, B, weighted)
    a, b = np.arange(len(j) - grid), np.arange(grid, len(j))
    to_partial = (nb[a] == PERM_BLOCK) & (nb[b] < PERM_BLOCK)
    to_short = (nl[a] == LIST_TILE) & (nl[b] < LIST_TILE)
    nan_first = np.array([names[q] in NAN_KINDS for q in j[a]])
    return {"block": int(to_partial.sum()), "tile": int(to_short.sum()), "from_nan": int(((to_partial | to_short) & nan_first).sum())}


def pair_kinds(names, listnan):
    """the (kind, list is NaN) of every pair of gsea_obs_kernel / gsea_edge_kernel in pair order e = l m + j"""
    return [(k, bool(bad)) for bad in listnan for k in names]


# ---- the references, on the K distinct lists ---------------------------------------------------------------------------------------
_REF = {}


def _once(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def ks_case():
    """(X, Gp, Gi) of the K lists of KS_KINDS for replaid.ssgsea.exact(single = FALSE), replaid.gsva.exact and
    replaid.sing.exact"""
    return _once("ks_case", lambda: (columns(),) + kinds_pattern(KS_KINDS))


def ssgsea_ks_ref(alpha):
    """K x NCOL: gsea_ks_walk.candidates_max_dev (scale = TRUE)"""
    from . import gsea_ks_walk as kw
    return _once(("ssgsea", alpha), lambda: kw.candidates_max_dev(*ks_case(), alpha, True))


def gsva_ks_ref(tau, max_diff):
    """K x NCOL: gsva_walk.pinned on rowtf = "none" """
    from . import gsva_walk as gw
    return _once(("gsva", tau, max_diff), lambda: gw.pinned(*ks_case(), tau, max_diff))


def sing_ref():
    """{name: K x NCOL}: sing_mad.pinned, up sets only"""
    from . import sing_mad as sm
    return _once("sing", lambda: sm.pinned(*ks_case()))


def gsea_case(ncol, nan_lists, weighted, B):
    """(stat, weight, P, Gp, Gi of the K lists of GSEA_KINDS, {score type: (out, null, le_len, le_idx)} by
    gsea_edge_ref.gsea_scored_ref) of one plaid.gsea call"""
    from . import gsea_edge_ref as er

    def make():
        stat, w, P = columns(ncol, nan_lists), gsea_weights(ncol, weighted), placements(B)
        Gp, Gi = kinds_pattern(GSEA_KINDS)
        return stat, w, P, Gp, Gi, er.gsea_scored_ref(stat, w, Gp, Gi, P)
    return _once(("gsea", ncol, tuple(nan_lists), weighted, B), make)


def expand_gsea(want, Gp_kinds, idx):
    """(out, null, le_len, le_idx) of the deck from the K lists' reference; padj (Benjamini-Hochberg over the sets of a list)
    is taken again over the deck's sets"""
    from . import gsea_perm_ref as ref
    w_out, w_null, w_len, w_idx = want
    out = np.asfortranarray(expand(w_out, idx))
    for l in range(out.shape[2]):
        out[:, 3, l] = ref.bh(out[:, 2, l])
    return out, np.asfortranarray(expand(w_null, idx)), np.asfortranarray(expand(w_len, idx)), expand_segments(w_idx, Gp_kinds, idx)
