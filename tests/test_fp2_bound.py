"""The input bound of the row-wise lazy Fp2 product and square (bls/field.hpp fp2_mul_rows /
fp2_sqr_rows, the bodies of the device's out-of-line fp2_mul_w / fp2_sqr_w): every
coefficient < 2p, so the tower's unreduced Karatsuba sums go in as they are.

* the column offset C2W_COL regenerated: a multiple of p whose column k dominates the
  largest column k of a1 b1 for digits 0..12 < 2^28 and digit 13 <= (2p - 1) >> 364;
* the algorithm restated on Python integers, column by column, at the extreme digit
  patterns: after every multiply-add every column is in [0, 2^64) (the device's columns are
  unsigned 64-bit registers and the reduction reads them as unsigned), and each coefficient
  is below 2p before the one conditional subtraction;
* the CPU build of the same source at the bound, word for word.
"""
from __future__ import annotations

import ctypes
import itertools
import random
from pathlib import Path

import pytest

from tests._codec import P

R = 1 << 384
R_INV = pow(R, -1, P)
M28 = (1 << 28) - 1
NP28 = (-pow(P, -1, 1 << 28)) % (1 << 28)
P28 = [(P >> (28 * k)) & M28 for k in range(14)]
BOUND = 2 * P  # exclusive
DMAX = [M28] * 13 + [(BOUND - 1) >> 364]  # the largest digit at every position
FIELD_HPP = Path(__file__).resolve().parent.parent / "lodestar_amd" / "csrc" / "bls" / "field.hpp"


def c2w_cols() -> list[int]:
    maxcol = [sum(DMAX[i] * DMAX[k - i] for i in range(14) if 0 <= k - i < 14) for k in range(27)]
    delta = (-sum(c << (28 * k) for k, c in enumerate(maxcol))) % P
    return [c + (((delta >> (28 * k)) & M28) if k < 14 else 0) for k, c in enumerate(maxcol)]


def digits(v: int) -> list[int]:
    assert 0 <= v < 1 << 384
    return [(v >> (28 * k)) & M28 for k in range(14)]  # digit 13: the top 20 bits


class Cols:
    """27 columns that must stay inside an unsigned 64-bit register after every step"""

    def __init__(self, init):
        self.t = list(init)
        self.lo, self.hi = min(self.t), max(self.t)

    def mac(self, k, prod):
        self.t[k] += prod
        assert 0 <= self.t[k] < 1 << 64, f"column {k} leaves [0, 2^64): {self.t[k]:#x}"
        self.lo, self.hi = min(self.lo, self.t[k]), max(self.hi, self.t[k])

    def redc(self) -> int:
        """fp_redc_rows + fp_d28_tail: the value / 2^384, below 2p"""
        t = self.t
        for i in range(14):
            m = (t[i] * NP28) & (M28 if i < 13 else 0xFFFFF)
            for j in range(14):
                self.mac(i + j, m * P28[j])
            if i < 13:
                assert (t[i] & M28) == 0
                self.mac(i + 1, t[i] >> 28)
                t[i] = 0
        assert (t[13] & 0xFFFFF) == 0
        v = sum(c << (28 * k) for k, c in enumerate(t))
        assert v % R == 0
        return v // R


def model_mul(x0, x1, y0, y1):
    c = Cols(c2w_cols())
    for i in range(14):
        for j in range(14):
            c.mac(i + j, x0[i] * y0[j])
        for j in range(14):
            c.mac(i + j, -(x1[i] * y1[j]))
    c0 = c.redc()
    d = Cols([0] * 27)
    for i in range(14):
        for j in range(14):
            d.mac(i + j, x0[i] * y1[j])
        for j in range(14):
            d.mac(i + j, x1[i] * y0[j])
    return c0, d.redc(), max(c.hi, d.hi)


def model_sqr(x0, x1):
    c = Cols(c2w_cols())
    for i in range(14):
        for j in range(i, 14):
            c.mac(i + j, x0[i] * (x0[j] if j == i else 2 * x0[j]))
        for j in range(i, 14):
            c.mac(i + j, -(x1[i] * (x1[j] if j == i else 2 * x1[j])))
    c0 = c.redc()
    d = Cols([0] * 27)
    for i in range(14):
        for j in range(14):
            d.mac(i + j, 2 * x0[i] * x1[j])
    return c0, d.redc(), max(c.hi, d.hi)


def val(d):
    return sum(x << (28 * k) for k, x in enumerate(d))


def test_offset_is_regenerated():
    cols = c2w_cols()
    assert sum(c << (28 * k) for k, c in enumerate(cols)) % P == 0 and max(cols) < 13 << 56
    src = FIELD_HPP.read_text()
    body = src[src.index("c2w_col(int k)"):]
    body = body[:body.index("return t[k]")]
    assert [int(w, 16) for w in __import__("re").findall(r"0x[0-9a-f]{16}(?=ull)", body)] == cols
    # the stated output bounds: (4 p^2 + C2W) / R + p and 8 p^2 / R + p
    c2w = sum(c << (28 * k) for k, c in enumerate(cols))
    assert ((BOUND - 1) ** 2 + c2w) // R + P < 1813 * P // 1000
    assert 2 * (BOUND - 1) ** 2 // R + P < 1813 * P // 1000


# digit patterns: nothing, the largest digit everywhere (above any value < 2p), the bound
# itself, p (digit 13 of 2p - 1 and of p differ), and all-ones low digits under a zero top
PATTERNS = [[0] * 14, DMAX, digits(BOUND - 1), digits(P), [M28] * 13 + [0], [0] * 13 + [DMAX[13]]]


def test_columns_stay_in_range_at_the_extremes():
    worst = 0
    for x0, x1, y0, y1 in itertools.product(PATTERNS, repeat=4):
        c0, c1, hi = model_mul(x0, x1, y0, y1)
        worst = max(worst, hi)
        a0, a1, b0, b1 = val(x0), val(x1), val(y0), val(y1)
        assert c0 < 2 * P and c1 < 2 * P
        assert c0 % P == (a0 * b0 - a1 * b1) * R_INV % P and c1 % P == (a0 * b1 + a1 * b0) * R_INV % P
    for x0, x1 in itertools.product(PATTERNS, repeat=2):
        c0, c1, hi = model_sqr(x0, x1)
        worst = max(worst, hi)
        a0, a1 = val(x0), val(x1)
        assert c0 < 2 * P and c1 < 2 * P
        assert c0 % P == (a0 * a0 - a1 * a1) * R_INV % P and c1 % P == 2 * a0 * a1 * R_INV % P
    assert worst < 1 << 62  # offset < 13 2^56, a b and m p < 14 2^56 each, the carry from below


def test_columns_stay_in_range_on_random_values():
    rng = random.Random(77)
    for _ in range(40):
        a0, a1, b0, b1 = (rng.randrange(BOUND) for _ in range(4))
        c0, c1, _ = model_mul(digits(a0), digits(a1), digits(b0), digits(b1))
        assert c0 < 2 * P and c0 % P == (a0 * b0 - a1 * b1) * R_INV % P
        assert c1 < 2 * P and c1 % P == (a0 * b1 + a1 * b0) * R_INV % P


@pytest.fixture(scope="module")
def rows_host():
    from lodestar_amd.build import build_fp2_rows_host

    return ctypes.CDLL(str(build_fp2_rows_host(verbose=False)))


def test_host_build_at_the_bound(rows_host):
    """the portable form of the very rows the device runs: canonical, exact output for
    coefficients up to 2p - 1"""
    rng = random.Random(78)
    o = ctypes.create_string_buffer(96)
    edge = [0, 1, R % P, P - 1, P, P + 1, BOUND - 1, BOUND - 2, 2 ** 381, BOUND - 2 ** 364, val([M28] * 13 + [0])]
    quads = [(e1, e2, e1, e2) for e1 in edge for e2 in edge] + [(e1, e2, e2, e1) for e1 in edge for e2 in edge]
    quads += [(0, BOUND - 1, 0, BOUND - 1), (BOUND - 1, 0, BOUND - 1, 0), (BOUND - 1,) * 4]
    quads += [tuple(rng.randrange(BOUND) for _ in range(4)) for _ in range(300)]
    for a0, a1, b0, b1 in quads:
        le = [v.to_bytes(48, "little") for v in (a0, a1, b0, b1)]
        rows_host.fr_fp2_mul_rows_raw(le[0] + le[1], le[2] + le[3], o)
        c0, c1 = int.from_bytes(o.raw[:48], "little"), int.from_bytes(o.raw[48:], "little")
        assert c0 == (a0 * b0 - a1 * b1) * R_INV % P, (a0, a1, b0, b1)
        assert c1 == (a0 * b1 + a1 * b0) * R_INV % P, (a0, a1, b0, b1)
        rows_host.fr_fp2_sqr_rows_raw(le[0] + le[1], o)
        c0, c1 = int.from_bytes(o.raw[:48], "little"), int.from_bytes(o.raw[48:], "little")
        assert c0 == (a0 * a0 - a1 * a1) * R_INV % P, (a0, a1)
        assert c1 == 2 * a0 * a1 * R_INV % P, (a0, a1)
