"""Decks of columns for the rank kernels' column loops (host only: numpy + the C oracle).

The rank kernels carry state from one column to the next inside a workgroup: the bucket ranker's prefetched successor, its
histograms and hand-over flag, the sorting networks' LDS key area and NaN counter, the densify scratch column, the
partitioned ranker's LDS counters.  A launch with more columns than workgroups gives workgroup w the columns
w, w + grid, w + 2 grid, ...; `deck` deals column KINDS so that, over all workgroups, every kind is followed by every kind
(itself included) inside some workgroup.  `pairs_seen` restates which ordered pairs a given assignment produces for a given
grid, so that a test can assert its input has the property before it looks at the device.

A deck needs n - grid >= k * k successions for k kinds (196 for the 14 kinds): `deck` raises ValueError otherwise.  The GPU
tests deal trips * grid + 37 columns with trips = 2 or 3, which assumes a grid of some 80 workgroups or more (an MI355X
has 256 CUs).

Nothing here touches the GPU; tests/test_rank_decks_ref.py checks this file against scipy."""
import numpy as np

NAN = float("nan")

# the eleven kinds of _rank_cases (tests/test_gpu_parity.py), in its order, then the three this file adds
KINDS = ("continuous", "rounded", "zeros95", "constant", "two_clusters", "near_one", "specials", "nan1", "small_int",
         "lognormal", "ulp_steps", "all_nan", "one_valid", "forced")
FORCED_MIN_LEN = 259          # two outliers + 257 clustered keys: a mixed fine bucket above kFallbackCount = 256
CSC_LENGTHS = (0, 1, 2, 63, 64, 65, 257, 8192, 8193, 12289)     # + the longest column the test's route takes ("max")
DENSIFY_PATTERNS = ("empty", "one", "full", "sparse5")


def column(kind, g, rng):
    """one column of length g of the given kind"""
    if kind == "continuous":
        return rng.normal(8, 2, g)
    if kind == "rounded":
        return np.round(rng.normal(8, 2, g), 1)
    if kind == "zeros95":
        return np.where(rng.random(g) < 0.95, 0.0, np.round(rng.gamma(2.0, 1.0, g), 1))
    if kind == "constant":
        return np.full(g, 3.25)
    if kind == "two_clusters":
        return np.where(rng.random(g) < 0.5, 1e-300, 1e300) * rng.random(g)
    if kind == "near_one":
        return np.where(rng.random(g) < 0.5, 1.0, 1.0 + 1e-12 * rng.integers(0, 3, g))
    if kind == "specials":
        return rng.choice([-np.inf, np.inf, 0.0, -0.0, 5e-324, -5e-324, 1.0], g)
    if kind == "nan1":
        return np.where(rng.random(g) < 0.01, np.nan, rng.normal(0, 1, g))
    if kind == "small_int":
        return rng.integers(-3, 4, g).astype(float)
    if kind == "lognormal":
        return np.exp(rng.normal(0, 8, g))
    if kind == "ulp_steps":
        return 1.0 + rng.integers(0, 40, g) * 2.0 ** -52
    if kind == "all_nan":
        return np.full(g, np.nan)
    if kind == "one_valid":
        x = np.full(g, np.nan)
        if g > 0:
            x[int(rng.integers(0, g))] = -3.5
        return x
    if kind == "all_zero":                       # (for the column maxima of signed ranks: zeros of both signs)
        return np.where(rng.random(g) < 0.5, 0.0, -0.0)
    if kind == "zero_nan":
        return np.where(rng.random(g) < 0.1, np.nan, 0.0)
    if kind in ("forced", "forced_nan"):
        # rank_bucket.h: a key's fine bucket is a function of the top 32 bits of (key - lo) (PH_D32; the whole offset when
        # the column's key range is shorter).  The two outliers stretch the range over nearly all of the key space, the
        # four clustered values differ in the last two bits of their keys: one fine bucket holds g - 2 keys that are not
        # all equal, and beyond kFallbackCount = 256 of them the column goes to the sorting network.  |x| keeps the
        # property (the outliers become one tied maximum, lo becomes the key of 1.0): signed or not, any g >= 259.
        x = 1.0 + (np.arange(g) % 4) * 2.0 ** -52
        if g > 0:
            x[0] = -1e300
        if g > 1:
            x[1] = 1e300
        if kind == "forced_nan" and g > 2:       # the same hand-over with 1 % NaN among the clustered keys
            x[2:][rng.random(g - 2) < 0.01] = np.nan
        return x
    raise ValueError(kind)


def key_of(x, signed=False):
    """the bucket ranker's order-preserving u64 key of a non-NaN double (rank_bucket.h, step 1)"""
    x = np.asarray(x, dtype=np.float64)
    x = (np.abs(x) if signed else x) + 0.0                       # -0 -> +0
    u = x.view(np.uint64)
    neg = (u >> np.uint64(63)) != 0
    return np.where(neg, ~u, u | np.uint64(1 << 63))


def pair_cycle(k):
    """a cyclic sequence over range(k) of length k * k in which every ordered pair (a, b), a == b included, appears
    exactly once as neighbours (wrapping around): an Euler circuit of the complete digraph with loops (Hierholzer)"""
    if k <= 0:
        return []
    nxt = [0] * k                 # next unused successor of each node
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            circuit.append(stack.pop())
    circuit.reverse()             # k * k + 1 nodes, first == last
    return circuit[:-1]


def _deal(items, grid, n):
    """item of each of n columns: the columns of workgroup w, c == w (mod grid), follow consecutive entries of
    pair_cycle(len(items)); workgroup w starts where workgroup w - 1 stopped, so that the pairs met by all workgroups
    together are the first n - grid pairs of the cycle"""
    items = list(items)
    k = len(items)
    if n - grid < k * k:
        raise ValueError(f"{n} columns on a grid of {grid} give {max(n - grid, 0)} successions: fewer than the {k * k} "
                         f"ordered pairs of {k} kinds")
    cyc = pair_cycle(k)
    out = [None] * n
    off = 0
    for w in range(min(grid, n)):
        cols = range(w, n, grid)
        for t, c in enumerate(cols):
            out[c] = items[cyc[(off + t) % (k * k)]]
        off += len(cols) - 1
    return out


def deck(kinds, grid, trips, tail):
    """the kind of each of n = trips * grid + tail columns (see the module docstring); ValueError when the launch is too
    short to show every ordered pair"""
    return _deal(kinds, grid, trips * grid + tail)


def pairs_seen(kind_of_column, grid):
    """the ordered pairs (kind of a column, kind of the next column of the same workgroup) of a launch on `grid` workgroups"""
    n = len(kind_of_column)
    return {(kind_of_column[c], kind_of_column[c + grid]) for c in range(n - grid)}


def all_pairs(kinds):
    return {(a, b) for a in kinds for b in kinds}


def dense_deck(kind_of_column, g, seed):
    """g x n matrix (Fortran order) with one column per entry of kind_of_column"""
    rng = np.random.default_rng(seed)
    X = np.empty((g, len(kind_of_column)), order="F")
    for c, kind in enumerate(kind_of_column):
        X[:, c] = column(kind, g, rng)
    return X


def ranks_ref(X, ties="average", signed=False):
    """colranks of a dense matrix by the C oracle: the NaN-free columns in one call; a column with NaN gets the oracle on
    its valid rows and NaN elsewhere (the oracle takes NaN-free vectors only)"""
    from oracle import c_oracle
    X = np.asfortranarray(X, dtype=np.float64)
    R = np.full(X.shape, np.nan, order="F")
    bad = np.isnan(X).any(axis=0)
    clean = np.flatnonzero(~bad)
    if len(clean) and X.shape[0] > 0:
        R[:, clean] = c_oracle.colranks_dense(X[:, clean], ties, signed)
    for c in np.flatnonzero(bad):
        ok = ~np.isnan(X[:, c])
        if ok.any():
            R[ok, c] = c_oracle.colranks_dense(X[ok, c:c + 1], ties, signed)[:, 0]
    return R


def csc_ranks_ref(Xp, Xx, ties="average", signed=False):
    """sparse_colranks of the stored values by the C oracle: one call on the columns with their NaN entries taken out, NaN
    at those entries"""
    from oracle import c_oracle
    Xp = np.asarray(Xp, dtype=np.int64)
    Xx = np.asarray(Xx, dtype=np.float64)
    ok = ~np.isnan(Xx)
    kept = np.concatenate([[0], np.cumsum(ok)])[Xp]               # column pointers of the NaN-free copy
    R = np.full(len(Xx), np.nan)
    if ok.any():
        R[ok] = c_oracle.sparse_colranks(kept.astype(np.int32), Xx[ok], ties, signed)
    return R


def csc_lengths(max_len, grid, trips, tail):
    """stored-value counts of n = trips * grid + tail CSC columns: CSC_LENGTHS and max_len, every ordered pair of lengths
    in some workgroup"""
    return _deal([v for v in CSC_LENGTHS if v < max_len] + [max_len], grid, trips * grid + tail)


def csc_values(lengths, kind_of_column, seed):
    """(Xp int32, Xx) of CSC columns with the given numbers of stored values, column c of kind kind_of_column[c]"""
    rng = np.random.default_rng(seed)
    Xp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    Xx = np.empty(int(Xp[-1]))
    for c, (k, kind) in enumerate(zip(lengths, kind_of_column)):
        Xx[Xp[c]:Xp[c + 1]] = column(kind, int(k), rng)
    return Xp, Xx


def densify_deck(pattern_of_column, kind_of_column, g, seed):
    """(Xp, Xi, Xx) of a g-row CSC matrix for the densify-and-rank route: per column one of DENSIFY_PATTERNS -- no stored
    value, one, all g rows stored, or about 5 % of the rows with stored zeros and negatives among them; the stored values of
    column c are of kind kind_of_column[c]"""
    rng = np.random.default_rng(seed)
    rows, vals, lens = [], [], []
    for pat, kind in zip(pattern_of_column, kind_of_column):
        if pat == "empty":
            r = np.empty(0, dtype=np.int32)
        elif pat == "one":
            r = rng.integers(0, g, 1).astype(np.int32)
        elif pat == "full":
            r = np.arange(g, dtype=np.int32)
        elif pat == "sparse5":
            r = np.flatnonzero(rng.random(g) < 0.05).astype(np.int32)
        else:
            raise ValueError(pat)
        v = column(kind, len(r), rng)
        if pat == "sparse5" and len(r) >= 4:
            v[0] = 0.0                                            # stored zeros stay stored ...
            v[len(r) // 2] = -0.0
            v[1] = -abs(v[1]) if v[1] == v[1] else -1.5           # ... and negatives rank below the implicit zeros
            v[-1] = -2.5
        rows.append(r)
        vals.append(v)
        lens.append(len(r))
    Xp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return Xp, np.concatenate(rows).astype(np.int32), np.concatenate(vals).astype(np.float64)


def csc_toarray(Xp, Xi, Xx, g):
    """the dense g x n matrix (Fortran order) of CSC arrays with unique rows per column; stored NaN stay NaN"""
    n = len(Xp) - 1
    X = np.zeros((g, n), order="F")
    cols = np.repeat(np.arange(n), np.diff(Xp))
    X[Xi, cols] = Xx
    return X
