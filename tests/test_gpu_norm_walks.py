"""normalize_medians' two passes over S (col_medians, shift_columns) at the shapes where a walk order, a prefetch or a
reordered end of the selection could go wrong -- `pytest -m gpu`.

Every case goes medians -> sum -> shift once through the C ABI on device memory laid out by the test: a leading dimension
above m, S starting 8 bytes into the allocation (8- but not 16-byte aligned), the last column ending exactly where a guard
column begins.  The medians equal the C oracle's, the shifted matrix is (x - med) + add bit for bit, nothing outside the
m x n values is written, nothing read behind the last column changes a result, and a permutation of the columns permutes
the medians."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from oracle import c_oracle
from tests.helpers import exact_ref as er

pytestmark = pytest.mark.gpu

# col_medians_wave_kernel's instantiations hold ITEMS rows of 64 values and read the first ITEMS - 16 of them unmasked
ITEMS = (16, 32, 48, 64, 80, 96)
M_SIZES = sorted({1, 2, 63, 64, 65, 1024, 1025, 4096, 4097, 5000, 5120, 6143, 6144, 6145}
                 | {64 * (it - 16) + d for it in ITEMS for d in (-1, 0, 1) if 64 * (it - 16) + d > 0})
N_SIZES = (1, 2, 3, 7, 9, 1025)
PAD_SENTINEL = 12345.0

KINDS = ("normal", "equal", "two", "ties", "nan", "one", "zeros", "signed_zeros", "inf", "denormal", "same_high",
         "normal_zeros", "neg_zero_mix")


def _block(kind, m, k, rng):
    """k columns of length m of one kind"""
    if kind == "normal":
        return rng.normal(size=(m, k))
    if kind == "equal":
        return np.full((m, k), 3.5) * rng.choice([-1.0, 1.0], size=(1, k))
    if kind == "two":
        return np.where(rng.random((m, k)) < 0.5, -1.25, 7.0)
    if kind == "ties":
        return np.round(rng.normal(size=(m, k)), 1)
    if kind == "nan":
        return np.full((m, k), np.nan)
    if kind == "one":
        b = np.full((m, k), np.nan)
        b[rng.integers(0, m, size=k), np.arange(k)] = rng.normal(size=k)
        return b
    if kind == "zeros":
        return np.zeros((m, k))
    if kind == "signed_zeros":
        return np.where(rng.random((m, k)) < 0.5, 0.0, -0.0)
    if kind == "inf":
        # 30 % +inf and 25 % -inf at random rows: the median stays finite (an infinite one would turn the mean of the
        # medians, and with it the whole shifted matrix, into NaN and leave the shift unchecked)
        b = rng.normal(size=(m, k))
        r = rng.random((m, k)).argsort(axis=0).argsort(axis=0)
        b[r < (int(0.3 * m) if m >= 4 else 0)] = np.inf
        b[r >= m - int(0.25 * m)] = -np.inf
        return b
    if kind == "denormal":
        return rng.integers(-2000, 2000, size=(m, k)).astype(np.float64) * 5e-324
    if kind == "same_high":                                    # 1 + j 2^-52, j < 2^32: one high dword, 0x3ff00000
        return 1.0 + rng.integers(0, 2 ** 32, size=(m, k)).astype(np.float64) * 2.0 ** -52
    if kind == "normal_zeros":
        b = rng.normal(size=(m, k))
        b[rng.random((m, k)) < 0.4] = 0.0
        return b
    b = np.abs(np.round(rng.normal(size=(m, k)), 1))            # neg_zero_mix: values >= 0 with both zeros among them
    z = b == 0.0
    b[z & (rng.random((m, k)) < 0.5)] = -0.0
    return b


def _matrix(m, n, seed):
    """m x n, column c of kind (c + m) mod |KINDS|; every second round of kinds loses its first value to a NaN, so both
    parities of the valid count occur for every kind that has one"""
    rng = np.random.default_rng(seed)
    S = np.empty((m, n), order="F")
    cols = np.arange(n)
    for q, kind in enumerate(KINDS):
        idx = cols[(cols + m) % len(KINDS) == q]
        if len(idx):
            S[:, idx] = _block(kind, m, len(idx), rng)
    flip = cols[(((cols // len(KINDS)) % 2) == 1) & ((cols + m) % len(KINDS) != KINDS.index("one"))]   # ("one" keeps its value)
    if m > 1 and len(flip):
        S[0, flip] = np.nan
    return S


class _Device:
    """device buffers of one case, through plaidhip_malloc / memcpy"""

    def __init__(self, ctx):
        self.ctx, self.lib, self.ptrs = ctx, ctx.lib, []

    def _check(self, rc):
        assert rc == 0, self.lib.plaidhip_last_error_string()

    def alloc(self, nbytes):
        p = C.c_void_p()
        self._check(self.lib.plaidhip_malloc(self.ctx.handle, C.c_size_t(nbytes), C.byref(p)))
        self.ptrs.append(p)
        return p.value

    def put(self, dst, arr):
        arr = np.ascontiguousarray(arr)
        self._check(self.lib.plaidhip_memcpy_h2d(self.ctx.handle, C.c_void_p(dst), C.c_void_p(arr.ctypes.data),
                                                 C.c_size_t(arr.nbytes)))

    def get(self, src, count, dtype=np.float64):
        out = np.empty(count, dtype=dtype)
        self._check(self.lib.plaidhip_memcpy_d2h(self.ctx.handle, C.c_void_p(out.ctypes.data), C.c_void_p(src),
                                                 C.c_size_t(out.nbytes)))
        return out

    def close(self):
        for p in self.ptrs:
            self.lib.plaidhip_free(self.ctx.handle, p)
        self.ptrs = []


def _pipeline(ctx, S, lds, head, iz, flag_words=None, guard=np.nan):
    """medians -> sum -> shift of S (m x n) stored with leading dimension lds, `head` doubles into its allocation, the
    last column ending where a guard column of lds doubles begins.  Returns (medians, {sum, count}, shifted m x n); asserts
    that the padding rows, the head and the guard come back untouched."""
    m, n = S.shape
    body = (n - 1) * lds + m
    total = head + body + lds
    host = np.full(total, PAD_SENTINEL)
    for c in range(n):
        host[head + c * lds: head + c * lds + m] = S[:, c]
    host[head + body:] = guard
    dev = _Device(ctx)
    try:
        base = dev.alloc(total * 8)
        d_med, d_red, d_flags = dev.alloc(n * 8), dev.alloc(4 * 8), dev.alloc(4 * 4)
        dev.put(base, host)
        dev.put(d_med, np.full(n, -777.0))
        dev.put(d_red, np.zeros(4))
        dev.put(d_flags, np.asarray(flag_words if flag_words is not None else (0, 0, 0, 0), dtype=np.uint32))
        p = base + 8 * head
        ctx.dev_col_medians(p, lds, m, n, iz, d_med, d_flags)
        ctx.dev_sum(d_med, n, d_red)
        ctx.dev_shift_columns(p, lds, m, n, d_med, 0.0, d_red)
        ctx.synchronize()
        med, red, back = dev.get(d_med, n), dev.get(d_red, 2), dev.get(base, total)
    finally:
        dev.close()
    out = np.empty((m, n), order="F")
    keep = np.ones(total, dtype=bool)
    for c in range(n):
        out[:, c] = back[head + c * lds: head + c * lds + m]
        keep[head + c * lds: head + c * lds + m] = False
    er.assert_same_bits(back[keep], host[keep], "values outside the m x n matrix")
    return med, red, out


def _same(a, b):
    """== with NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _check_case(S, med, red, out, exp, what):
    """exp: the C oracle's medians of S"""
    assert _same(med, exp), (what, np.flatnonzero(~((med == exp) | (np.isnan(med) & np.isnan(exp))))[:5])
    ok = ~np.isnan(med)
    assert red[1] == ok.sum(), what
    with np.errstate(all="ignore"):
        add = red[0] / red[1]                                  # the kernel's own division, fp64 on both sides
        fm = med[ok]
        if ok.any() and np.isfinite(fm).all():
            exact = float(sum((Fraction(float(v)) for v in fm), Fraction(0)) / len(fm))
            # a sum of cnt medians (cnt - 1 roundings) and the division: (cnt + 2) u mean|med|
            assert abs(add - exact) <= (len(fm) + 2) * er.U * np.abs(fm).mean() + 2.0 ** -1074, (what, add, exact)
        er.assert_same_bits(out, (S - med[None, :]) + add, what + ": shifted matrix")


# ignore_zero as passed, the flag words {has-negative, has-zero} beside it, and what the oracle is told
MODES = ((False, None, False), (True, None, True),
         (None, (0, 1, 0, 0), True),       # zeros and no negative value: min(x) == 0
         (None, (1, 1, 0, 0), False),      # zeros below a negative minimum
         (None, (0, 0, 0, 0), False))      # no zero at all


@pytest.mark.parametrize("n", N_SIZES)
@pytest.mark.parametrize("m", M_SIZES)
def test_medians_sum_shift_on_an_offset_padded_matrix(hip_ctx, m, n):
    """every column kind at every boundary of the kernels' size classes and grids: medians == the C oracle's, the shifted
    matrix (x - med) + add bit for bit, nothing written outside it; the guard column behind S changes nothing; permuted
    columns give permuted medians"""
    S = _matrix(m, n, 1000 * m + n)
    lds, head = m + 3, 1                                        # odd and even m: columns of both alignments
    first = None
    oracle = {z: c_oracle.normalize_medians(S, z)[1] for z in (False, True)}     # once per case, shared by the modes
    for iz, words, iz_oracle in MODES:
        med, red, out = _pipeline(hip_ctx, S, lds, head, iz, words)
        _check_case(S, med, red, out, oracle[iz_oracle], f"m={m} n={n} iz={iz} flags={words}")
        if first is None:
            first = (med, red, out)
    # the guard column's contents (all that lies behind the last column) must not matter
    rng = np.random.default_rng(m + n)
    med_g, red_g, out_g = _pipeline(hip_ctx, S, lds, head, False, None, guard=rng.normal(size=lds) * 1e300)
    er.assert_same_bits(med_g, first[0], "medians with another guard column")
    er.assert_same_bits(red_g, first[1], "sum with another guard column")
    er.assert_same_bits(out_g, first[2], "shifted matrix with another guard column")
    # lds == m, 16-byte aligned, columns permuted: the same medians, permuted
    perm = rng.permutation(n)
    Sp = np.asfortranarray(S[:, perm])
    med_p, red_p, out_p = _pipeline(hip_ctx, Sp, m, 0, False, None)
    er.assert_same_bits(med_p, first[0][perm], "medians of the permuted columns")
    _check_case(Sp, med_p, red_p, out_p, oracle[False][perm], f"m={m} n={n} permuted")
