"""Vectors and exact references of the device field-op self-test
(include/lodestar_bls.h bls_gpu_field_op_test, kernels/field_ops.hpp).

One VectorSet per op: its records (tuples of Python integers), how a record packs into
32-bit words, and a check of the device's output words against Python integers --
exact, no tolerances.  The contract checked is the function's own comment in
csrc/bls/*.hpp; "canonical" means < p.  Each set holds the edges at which carry chains
and lazy bounds go wrong plus 300 seeded random operands over the op's full input
range, and its length is never a multiple of 64 (the tail wavefront is partial).

tests/test_gpu_field_ops.py runs the sets on the GPU; tests/test_fieldvec.py runs the
same records and references through the CPU build of the same headers
(tests/native/hostsim.cpp), so a wrong reference shows without a GPU."""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from typing import Callable

from tests._codec import P

R = 1 << 384
R_INV = pow(R, -1, P)
RP_INV = pow(2, -392, P)  # lazy28's R' = 2^392
M28 = (1 << 28) - 1
D28 = 0x100  # BLS_FIELD_OP_D28
N_RANDOM = 300

# base op ids (csrc/kernels/field_ops.hpp FOP_*)
(ADD, SUB, NEG, DBL, HALF, ADD_NR, SUB_NR, REDUCE_ONCE, REDUCE_2P, CANON3, MUL, SQR, MUL_LAZY, SQR_D28_LAZY,
 FP2_MUL_D28, FP2_SQR_D28, FP2_MUL, FP2_SQR, FP2_MUL_S, LZ_MUL_RAW, LZ_SQR_RAW, LZ_FP_OPS, LZ_FP2_OPS, INV, INV_GCD,
 SQRT, FP2_INV, FP2_SQRT, LIN8) = range(29)
PREDS = 32  # after the three fp2_*_prim ops of tests/test_gpu_fp2_prim.py (29..31)


def limbs(v: int, n: int = 12) -> list[int]:
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def unlimbs(w) -> int:
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def mont(v: int) -> int:
    return v * R % P


def unmont(v: int) -> int:
    return v * R_INV % P


def hx(rec) -> str:
    return "(" + ", ".join(hx(v) if isinstance(v, (tuple, list)) else hex(v) for v in rec) + ")"


@dataclass
class VectorSet:
    name: str
    op: int
    d28_only: bool
    records: list
    pack: Callable  # record -> list of uint32 words
    check: Callable  # (record, output words as Python ints) -> None or a description of the mismatch
    flavours: tuple = field(init=False)

    def __post_init__(self):
        self.flavours = (D28,) if self.d28_only else (0, D28)
        if len(self.records) % 64 == 0:  # keep the last wavefront partial
            self.records = self.records + [self.records[0]]
        assert len(self.records) < 1000


def _pack_fp(rec):
    return [w for v in rec for w in limbs(v)]


def _fps(words, n):
    return [unlimbs(words[12 * k: 12 * k + 12]) for k in range(n)]


# ---- carry chains ---------------------------------------------------------------------
def carry_pairs(rng) -> list:
    """canonical (a, b): a + b in {p-1, p, p+1, 2p-2}, a == b, (0, 1), (0, p-1), and carries
    / borrows that ripple through exactly k limbs, k = 1..11, both operand orders"""
    h = (P - 1) // 2
    pairs = [(0, P - 1), (h, h), (1, P - 2), (1, P - 1), (h, h + 1), (h + 1, h), (2, P - 1), (h + 1, h + 1),
             (P - 1, P - 1), (P - 1, 1), (P - 1, 2)]
    for s in (P - 1, P, P + 1, 2 * P - 2):
        for _ in range(4):
            a = rng.randrange(max(0, s - (P - 1)), min(P - 1, s) + 1)
            pairs.append((a, s - a))
    pairs += [(0, 0), (1, 1), (2, 2), (0, 1), (1, 0), (P - 1, 0)]
    pairs += [(v, v) for v in (rng.randrange(P) for _ in range(4))]
    for k in range(1, 12):
        for a, b in (((1 << (32 * k)) - 1, 1), (1 << (32 * k), 1)):
            pairs += [(a, b), (b, a)]
    pairs += [(rng.randrange(P), rng.randrange(P)) for _ in range(N_RANDOM)]
    assert all(a < P and b < P for a, b in pairs)
    return pairs


def carry_singles(rng, bound: int, edges) -> list:
    vals = list(edges) + [(1 << (32 * k)) - 1 for k in range(1, 12)] + [1 << (32 * k) for k in range(1, 12)]
    vals += [rng.randrange(bound) for _ in range(N_RANDOM)]
    assert all(0 <= v < bound for v in vals)
    return [(v,) for v in vals]


def _eq1(name, want_of):
    def check(rec, out):
        got, want = unlimbs(out[:12]), want_of(*rec)
        if got != want:
            return f"{name}{hx(rec)} = {got:#x}, want {want:#x}"
    return check


# ---- products ---------------------------------------------------------------------------
LAZY_EDGES = [0, 1, P - 1, P, 2 * P - 1, 3 * P - 1, 2 ** 382, 3 * P - 2 ** 200]  # test_fp_mul_d28_lazy
BOUND_PAIRS = [(2 * P - 1, 4 * P - 1), (2 * P - 1, 4 * P - 2 ** 100), (P, 4 * P - 1), (0, 4 * P - 1)]  # .._input_bound
CANON_EDGES = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, 2 ** 380, R % P]
FP2_EDGES = [0, 1, P - 1, P - 2, (P - 1) >> 1, 2 ** 380, P - 2 ** 364]  # test_fp2_mul_lazy
FP2S_EDGES = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P - 2, 2 ** 381]  # test_fp2_mul_s


def _strided(vals, k):
    return vals[k], vals[(k * 5 + 1) % len(vals)], vals[(k * 11 + 2) % len(vals)], vals[(k * 3 + 4) % len(vals)]


def fp2_quads(rng, edges, bound) -> list:
    """(a0, a1, b0, b1): the edge list crossed so that (0, p-1, 0, p-1) -- the largest
    a1 b1 on the smallest a0 b0, the bottom of the C2_COL offset -- and (p-1, 0, p-1, 0)
    both occur, the strided walk of test_fp2_mul_lazy, and random operands"""
    quads = [(e1, e2, e1, e2) for e1 in edges for e2 in edges] + [(e1, e2, e2, e1) for e1 in edges for e2 in edges]
    vals = edges + [rng.randrange(bound) for _ in range(N_RANDOM)]
    quads += [_strided(vals, k) for k in range(len(vals))]
    assert (0, P - 1, 0, P - 1) in quads and (P - 1, 0, P - 1, 0) in quads
    return quads


def _check_mul(name, lazy):
    def check(rec, out):
        a, b = rec if len(rec) == 2 else (rec[0], rec[0])
        got = unlimbs(out[:12])
        if got >= (2 * P if lazy else P):
            return f"{name}{hx(rec)} = {got:#x} is not below {'2p' if lazy else 'p'}"
        if got % P != a * b * R_INV % P:
            return f"{name}{hx(rec)} = {got:#x}, want {a * b * R_INV % P:#x} (mod p)"
    return check


def _check_fp2(name, want_of):
    def check(rec, out):
        c0, c1 = _fps(out, 2)
        w0, w1 = want_of(*rec)
        if (c0, c1) != (w0 % P, w1 % P):
            return f"{name}{hx(rec)} = ({c0:#x}, {c1:#x}), want ({w0 % P:#x}, {w1 % P:#x})"
    return check


def _fp2_mul_ref(a0, a1, b0, b1):
    return (a0 * b0 - a1 * b1) * R_INV, (a0 * b1 + a1 * b0) * R_INV


def _fp2_sqr_ref(a0, a1):
    return (a0 * a0 - a1 * a1) * R_INV, 2 * a0 * a1 * R_INV


# ---- lazy28 -------------------------------------------------------------------------------
def digits_value(d) -> int:
    return sum(int(x) << (28 * k) for k, x in enumerate(d))


def signed_digits(v: int, rng, dmax: int) -> list[int]:
    """A signed digit vector of value v (any sign) with |digits| pushed up to dmax (moving
    multiples of 2^28 between neighbouring digits), so the product sees unnormalised,
    mixed-sign operands."""
    d = [0] * 14
    m = abs(v)
    for k in range(13):
        d[k] = (m >> (28 * k)) & M28
    d[13] = m >> (28 * 13)
    if v < 0:
        d = [-x for x in d]
    for k in range(13):
        # move t units of digit k+1 into digit k (value unchanged)
        for _ in range(3):
            t = rng.randint(-4, 4)
            nk, nk1 = d[k] + t * (1 << 28), d[k + 1] - t
            if abs(nk) <= dmax and abs(nk1) <= dmax:
                d[k], d[k + 1] = nk, nk1
    assert digits_value(d) == v and max(abs(x) for x in d) <= dmax
    return d


def lz_raw_cases() -> list:
    """(x digits, y digits, value of x, value of y): operands at the largest digits
    lz_mul_fits admits (|digit| ~2^29.5 each side) and large magnitudes of either sign"""
    rng = random.Random(392)
    cases = []
    for _ in range(300):
        vx = rng.randrange(1 << rng.choice((10, 200, 381, 384, 388))) * rng.choice((1, -1))
        vy = rng.randrange(1 << rng.choice((10, 200, 381, 384, 388))) * rng.choice((1, -1))
        cases.append((vx, vy))
    cases += [(0, 0), (P - 1, P - 1), (-(2 * P - 1), 2 * P - 1), (256 * P - 1, -9 * P), ((1 << 388) - 1, P)]
    dmax = int(2 ** 29.5)
    out = []
    for vx, vy in cases:
        x = signed_digits(vx, rng, dmax)
        y = signed_digits(vy, rng, dmax)
        out.append((tuple(x), tuple(y), vx, vy))
    return out


def lz_raw_check(r, vx, vy):
    """the three assertions of test_lazy28_raw_product_bounds on output digits r, as a
    description of the first that fails (None: all hold)"""
    if not all(0 <= c <= M28 for c in r[:13]):
        return f"digits 0..12 not in [0, 2^28): {list(r)}"
    rv = digits_value(r)
    if rv % P != (vx * vy * RP_INV) % P:
        return f"value {rv:#x} is not x y / 2^392 (mod p)"
    if not abs(rv) < P + abs(vx * vy) // (1 << 392) + 1:
        return f"|value| {abs(rv):#x} is not below p + |x y| / 2^392"


def _s32(w):
    return [int(x) - (1 << 32) if int(x) >> 31 else int(x) for x in w]


def _check_lz_raw(sqr):
    def check(rec, out):
        x, y, vx, vy = rec
        err = lz_raw_check(_s32(out[:14]), vx, vx if sqr else vy)
        if err:
            return f"{'lz_sqr_w' if sqr else 'lz_mul_w'} on x = {list(x)}{'' if sqr else f', y = {list(y)}'}: {err}"
    return check


def lz_fp_ref(a, b) -> list:
    """the ten values of bls/selftest_ops.hpp sf_lz_fp_ops for plain a, b"""
    ab = a * b % P
    return [ab, a * a % P, (a + b) % P, (a - b) % P, (-ab) % P, ab * pow(2, -1, P) % P, (-ab) % P,
            (2 * ab - b * b) * (b - a) % P, a, 4 * (2 * ab - 7 * b * b - 7 * a) % P]


def f2mul(x, y):
    return ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def lz_fp2_ref(a, b) -> list:
    """the six values of sf_lz_fp2_ops for plain a = (a0, a1), b = (b0, b1)"""
    m, bb = f2mul(a, b), f2mul(b, b)
    return [m, f2mul(a, a), ((m[0] - m[1]) % P, (m[0] + m[1]) % P), (m[0], (-m[1]) % P),
            ((m[0] - bb[0]) % P, (m[1] - bb[1]) % P), (m[0] * b[0] % P, m[1] * b[0] % P)]


LZ_FP_NAMES = ("a b", "a^2", "a + b", "a - b", "-(a b)", "a b / 2", "-(a b) normalised", "(2ab - b^2)(b - a)",
               "a round trip", "lz_reduce 4 (2ab - 7 b^2 - 7 a)")
LZ_FP2_NAMES = ("l2_mul", "l2_sqr", "l2_mul_xi", "l2_conj", "l2_sub", "l2_mul_fp")


def lz_fp_pairs(rng) -> list:
    vals = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, 2 ** 380, P - 3]
    vals += [rng.randrange(P) for _ in range(N_RANDOM)]
    return [(a, vals[(7 * k + 3) % len(vals)]) for k, a in enumerate(vals)]


def lz_fp2_pairs(rng) -> list:
    edge = [0, 1, P - 1, (P - 1) // 2]
    out = []
    for k in range(N_RANDOM + 16):
        a = (rng.choice(edge) if k < 16 else rng.randrange(P), rng.randrange(P) if k % 3 else rng.choice(edge))
        b = (rng.randrange(P), rng.choice(edge) if k % 5 == 0 else rng.randrange(P))
        out.append((a, b))
    return out


def _check_lz_fp(rec, out):
    """plain (a, b) went in as Montgomery forms; the outputs are canonical Montgomery forms"""
    got = _fps(out, 10)
    for k, (g, w) in enumerate(zip(got, lz_fp_ref(*rec))):
        if g >= P or unmont(g) != w:
            return f"lazy28 {LZ_FP_NAMES[k]} on{hx(rec)} = {g:#x}, want {mont(w):#x}"


def _check_lz_fp2(rec, out):
    got = _fps(out, 12)
    for k, w in enumerate(lz_fp2_ref(*rec)):
        g = (got[2 * k], got[2 * k + 1])
        if max(g) >= P or (unmont(g[0]), unmont(g[1])) != w:
            return f"lazy28 {LZ_FP2_NAMES[k]} on{hx(rec)} = {hx(g)}, want {hx((mont(w[0]), mont(w[1])))}"


# ---- inversions and square roots (Montgomery forms in and out) -----------------------------
def is_square(a: int) -> bool:
    return pow(a, (P - 1) // 2, P) in (0, 1)  # Euler's criterion


def f2_is_square(a) -> bool:
    return is_square((a[0] * a[0] + a[1] * a[1]) % P)  # a is a square in Fp2 iff its norm is one in Fp


def _check_inv(name, zero_ok):
    def check(rec, out):
        a, x = rec[0], unlimbs(out[:12])
        if x >= P:
            return f"{name}({mont(a):#x}) = {x:#x} is not canonical"
        if a == 0:
            return None if (zero_ok and x == 0) else f"{name}(0) = {x:#x}, want 0"
        if a * unmont(x) % P != 1:
            return f"{name}({mont(a):#x}) = {x:#x}: x * x^-1 != 1"
    return check


def _check_sqrt(rec, out):
    a, ok, r = rec[0], out[0], unlimbs(out[1:13])
    if bool(ok) != is_square(a):
        return f"fp_sqrt({mont(a):#x}) says {'root' if ok else 'no root'}, Euler's criterion says the opposite"
    if ok and (r >= P or unmont(r) ** 2 % P != a):
        return f"fp_sqrt({mont(a):#x}) = {r:#x}: root^2 != a"


def _check_fp2_inv(rec, out):
    a = rec
    x = _fps(out, 2)
    if max(x) >= P or f2mul(a, (unmont(x[0]), unmont(x[1]))) != (1, 0):
        return f"fp2_inv{hx((mont(a[0]), mont(a[1])))} = {hx(x)}: x * x^-1 != 1"


def _check_fp2_sqrt(rec, out):
    a, ok, r = rec, out[0], _fps(out[1:], 2)
    if bool(ok) != f2_is_square(a):
        return f"fp2_sqrt{hx((mont(a[0]), mont(a[1])))} says {'root' if ok else 'no root'}, Euler's criterion on the norm says the opposite"
    if ok and (max(r) >= P or f2mul((unmont(r[0]), unmont(r[1])), (unmont(r[0]), unmont(r[1]))) != tuple(a)):
        return f"fp2_sqrt{hx((mont(a[0]), mont(a[1])))} = {hx(r)}: root^2 != a"


def sqrt_inputs(rng) -> list:
    vals = [0, 1, 2, 4, P - 1, P - 4]
    vals += [pow(rng.randrange(P), 2, P) for _ in range(N_RANDOM // 2)] + [rng.randrange(P) for _ in range(N_RANDOM // 2)]
    assert {is_square(v) for v in vals} == {True, False}
    return [(v,) for v in vals]


def fp2_sqrt_inputs(rng) -> list:
    vals = [(0, 0), (1, 0), (5, 0), (P - 5, 0), (0, 7), (0, P - 7), (25, 0), (P - 25, 0)]  # the a1 == 0 branch, a0 == 0
    for _ in range(N_RANDOM // 2):
        x = (rng.randrange(P), rng.randrange(P))
        vals += [f2mul(x, x), (rng.randrange(P), rng.randrange(P))]
    assert {f2_is_square(v) for v in vals} == {True, False}
    return vals


# ---- LIN8: the interpreter's linear combination ---------------------------------------------
CMAX = 32767


def _lin8(xs, cs, n, single=0):
    xs, cs = list(xs) + [0] * (8 - len(xs)), list(cs) + [0] * (8 - len(cs))
    assert all(0 <= x < 3 * P for x in xs) and all(abs(c) <= CMAX for c in cs) and 0 <= n <= 8
    # acc_reduce's precondition (coop.hpp): the 2^20 p bias covers sum |c| x for x < 3p
    assert 3 * sum(abs(c) for c in cs[:n]) <= 1 << 20
    return (tuple(xs), tuple(cs), n, single)


def acc_reduce_model(total: int, q_minus: int = 1) -> int:
    """coop.hpp acc_reduce on the exact sum `total` of the terms (the 13-limb two's
    complement accumulator holds total - negs and the bias adds negs back): the quotient
    estimate in double precision exactly as the device computes it.  q_minus = 0 models
    the defect "q in place of q - 1"; a negative return is a wrapped, wrong result."""
    a = total + (P << 20)
    assert 0 <= a < 1 << 416
    l10, l11, l12 = (a >> 320) & 0xFFFFFFFF, (a >> 352) & 0xFFFFFFFF, a >> 384
    d = float(l12) * 18446744073709551616.0 + float(l11) * 4294967296.0 + float(l10)
    q = int(d * float.fromhex("0x1.3b06ba5e7993dp-61"))
    q = max(q - q_minus, 0)
    return a - q * P


def lin8_records(rng) -> list:
    top = 3 * P - 1
    recs = [_lin8([top] * 8, [CMAX] * 8, 8), _lin8([top] * 8, [-CMAX] * 8, 8),
            _lin8([top] * 8, [CMAX, -CMAX] * 4, 8), _lin8([top] * 8, [-CMAX, CMAX] * 4, 8)]
    for _ in range(6):  # x = (v, v + p, v + 2p), c = (2, -1, -1): -3p exactly; negated: +3p
        v = rng.randrange(P)
        recs += [_lin8([v, v + P, v + 2 * P], [2, -1, -1], 3), _lin8([v, v + P, v + 2 * P], [-2, 1, 1], 3),
                 _lin8([v + 2 * P, v, v + P, v, v + 2 * P, v + P], [-1, 2, -1, -2, 1, 1], 6),  # exactly 0
                 _lin8([v, v], [CMAX, -CMAX], 2), _lin8([v + P, v], [77, -77], 2)]  # 0 and 77 p
    recs += [_lin8([0] * 8, [CMAX] * 8, 8), _lin8([P, 2 * P, P], [1, 1, -3], 3), _lin8([P], [-1], 1)]
    # every n (lanes of one wavefront carry different n; nmax is the wavefront's largest)
    for n in range(9):
        for _ in range(3):
            recs.append(_lin8([rng.randrange(3 * P) for _ in range(8)], [rng.randint(-CMAX, CMAX) for _ in range(8)], n))
    # the one-(+1)-term case, by the short cut (single) and through the accumulator
    for v in (0, 1, P - 1, P, 2 * P, top, rng.randrange(3 * P), rng.randrange(3 * P)):
        recs += [_lin8([v], [1], 1, single=1), _lin8([v], [1], 1, single=0)]
    # sums a hair below an exact multiple of p (x = k p - 1, c > 0): a quotient estimate
    # one too large wraps below zero.  Kept: those on which the modelled estimate is not
    # below the true quotient, i.e. where "q" in place of "q - 1" goes negative.
    tight = []
    for _ in range(4000):
        if len(tight) >= 24:
            break
        n = rng.randint(1, 8)
        xs = [rng.choice((1, 2, 3)) * P - 1 for _ in range(n)]
        cs = [rng.randint(1, CMAX) for _ in range(n)]
        total = sum(c * x for c, x in zip(cs, xs))
        if acc_reduce_model(total, q_minus=0) < 0:
            tight.append(_lin8(xs, cs, n))
    recs += tight
    for _ in range(N_RANDOM):
        n = rng.randint(0, 8)
        small = rng.random() < 0.5
        cs = [rng.choice((-3, -2, -1, 1, 2, 3, 144)) if small else rng.randint(-CMAX, CMAX) for _ in range(8)]
        recs.append(_lin8([rng.randrange(3 * P) for _ in range(8)], cs, n))
    return recs


def _pack_lin8(rec):
    xs, cs, n, single = rec
    w = [x for v in xs for x in limbs(v)]
    w += [(cs[2 * k] & 0xFFFF) | ((cs[2 * k + 1] & 0xFFFF) << 16) for k in range(4)]
    return w + [n, single]


def lin8_total(rec) -> int:
    xs, cs, n, _ = rec
    return sum(c * x for c, x in zip(cs[:n], xs[:n]))


def _check_lin8(rec, out):
    xs, cs, n, single = rec
    got = unlimbs(out[:12])
    what = f"coop_lin(n = {n}, single = {single}, c = {list(cs[:n])}, x = {hx(xs[:n])})"
    if single and got != xs[0]:
        return f"{what} = {got:#x}, want the slot itself"
    if got >= 3 * P:
        return f"{what} = {got:#x} is not below 3p"
    if got % P != lin8_total(rec) % P:
        return f"{what} = {got:#x}, want {lin8_total(rec) % P:#x} (mod p)"


# ---- PREDS: the comparison predicates (bls/selftest_ops.hpp sf_preds) -----------------------
# One output word, one bit per predicate.  Bits 0..6 read the two input values as plain
# 384-bit integers and are defined (and checked) on ANY input.  Bits 7..11 read them as
# Montgomery forms c R mod p; they are defined on canonical input only, so a bit is
# checked only when every value it reads is below p.
PRED_BITS = ("fp_plain_is_canonical(c0)", "fp_plain_is_canonical(c1)", "fp_plain_gt_half(c0)", "fp_plain_gt_half(c1)",
             "fp_is_zero(c0)", "fp_is_zero(c1)", "fp_eq(c0, c1)", "fp_lex_largest(c0)", "fp_lex_largest(c1)",
             "fp2_lex_largest", "fp2_sgn0", "fp2_is_zero")
PRED_PLAIN_MASK = 0x7F


def preds_ref(c0: int, c1: int) -> tuple[int, int]:
    """(expected word, mask of the bits defined on this input) for raw values c0, c1"""
    h = (P - 1) // 2
    bits = [c0 < P, c1 < P, c0 > h, c1 > h, c0 == 0, c1 == 0, c0 == c1]
    mask = PRED_PLAIN_MASK
    p0, p1 = unmont(c0 % P), unmont(c1 % P)
    bits += [p0 > h, p1 > h, (p1 > h) if p1 != 0 else (p0 > h), (p0 & 1) | (int(p0 == 0) & (p1 & 1)),
             p0 == 0 and p1 == 0]
    if c0 < P:
        mask |= 1 << 7
    if c1 < P:
        mask |= 1 << 8
    if c0 < P and c1 < P:
        mask |= 7 << 9
    return sum(int(b) << k for k, b in enumerate(bits)), mask


def preds_records(rng) -> list:
    h = (P - 1) // 2
    plain = [0, 1, h, h + 1, P - 2, P - 1, P, P + 1, 2 * P - 1, 2 ** 381 - 1, 2 ** 384 - 1]
    for k in range(12):
        plain += [P + (1 << (32 * k)), P - (1 << (32 * k)), h + (1 << (32 * k)), h - (1 << (32 * k))]
    assert all(0 <= v < R for v in plain)
    recs = [(v, plain[(7 * k + 3) % len(plain)]) for k, v in enumerate(plain)]
    recs += [(plain[(5 * k + 1) % len(plain)], v) for k, v in enumerate(plain)]
    recs += [(v, v) for v in plain[:11]]  # fp_eq; and values that differ in one limb only
    recs += [(h, h ^ (1 << (32 * k))) for k in range(12)]
    # Montgomery forms of the values at which the sign predicates change, every pair of
    # them: c1 == 0 (the c0 fallback of fp2_lex_largest) and c0 == 0 (the z0 & s1 term of
    # fp2_sgn0) included
    edge = [mont(v) for v in (0, 1, 2, h, h + 1, P - 1)]
    recs += [(a, b) for a in edge for b in edge]
    recs += [(rng.randrange(P), 0) for _ in range(8)] + [(0, rng.randrange(P)) for _ in range(8)]
    for k in range(N_RANDOM):
        bound = P if k % 2 == 0 else R
        recs.append((rng.randrange(bound), rng.randrange(bound)))
    return recs


def _check_preds(rec, out):
    want, mask = preds_ref(*rec)
    diff = (out[0] ^ want) & mask
    if diff or out[0] >> len(PRED_BITS):
        bad = [f"{PRED_BITS[k]} = {out[0] >> k & 1}, want {want >> k & 1}" for k in range(len(PRED_BITS)) if diff >> k & 1]
        return f"predicates on{hx(rec)}: {'; '.join(bad) or 'bits set past the table'} (word {out[0]:#x})"


# ---- the sets -------------------------------------------------------------------------------
def build_sets() -> list[VectorSet]:
    rng = random.Random(0xF1E1D)
    pairs = carry_pairs(rng)
    canon1 = carry_singles(rng, P, [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2])
    lazy_vals = LAZY_EDGES + [rng.randrange(3 * P) for _ in range(N_RANDOM)]
    lazy_pairs = [(a, lazy_vals[(7 * k + 3) % len(lazy_vals)]) for k, a in enumerate(lazy_vals)]
    canon_vals = CANON_EDGES + [rng.randrange(P) for _ in range(N_RANDOM)]
    mul_pairs = [(a, canon_vals[(7 * k + 3) % len(canon_vals)]) for k, a in enumerate(canon_vals)]
    mul_pairs += [(a, a) for a in CANON_EDGES]
    # ... and at fp2_mul_s's bound: a < 2p, b < 4p (test_fp_mul_d28_input_bound)
    mul_pairs += BOUND_PAIRS + [(rng.randrange(2 * P), rng.randrange(4 * P)) for _ in range(N_RANDOM)]
    quads = fp2_quads(rng, FP2_EDGES, P)
    quads_s = fp2_quads(rng, FP2S_EDGES, 2 * P)
    sq_pairs = [(e1, e2) for e1 in FP2_EDGES for e2 in FP2_EDGES] + [(rng.randrange(P), rng.randrange(P))
                                                                    for _ in range(N_RANDOM)]
    raw = lz_raw_cases()
    inv_vals = [(v,) for v in [1, 2, 3, P - 1, P - 2, (P - 1) // 2, R % P] + [rng.randrange(1, P) for _ in range(N_RANDOM)]]
    fp2_inv_vals = [(1, 0), (0, 1), (P - 1, 0), (0, P - 1), (P - 1, P - 1), (1, 1)]
    fp2_inv_vals += [(rng.randrange(P), rng.randrange(P)) for _ in range(N_RANDOM)]

    def pack_mont(rec):
        return _pack_fp([mont(v) for v in rec])

    def pack_mont2(rec):  # ((a0, a1), (b0, b1)) plain -> Montgomery words
        return _pack_fp([mont(v) for c in rec for v in c])

    S = VectorSet
    return [
        S("fp_add", ADD, False, pairs, _pack_fp, _eq1("fp_add", lambda a, b: (a + b) % P)),
        S("fp_sub", SUB, False, pairs, _pack_fp, _eq1("fp_sub", lambda a, b: (a - b) % P)),
        S("fp_neg", NEG, False, canon1, _pack_fp, _eq1("fp_neg", lambda a: -a % P)),
        S("fp_dbl", DBL, False, canon1, _pack_fp, _eq1("fp_dbl", lambda a: 2 * a % P)),
        S("fp_half", HALF, False, canon1, _pack_fp, _eq1("fp_half", lambda a: a * pow(2, -1, P) % P)),
        S("fp_add_nr", ADD_NR, False, pairs, _pack_fp, _eq1("fp_add_nr", lambda a, b: a + b)),
        S("fp_sub_nr", SUB_NR, False, pairs, _pack_fp, _eq1("fp_sub_nr", lambda a, b: a + P - b)),
        S("fp_reduce_once", REDUCE_ONCE, False, carry_singles(rng, 2 * P, [0, P - 1, P, P + 1, 2 * P - 1]), _pack_fp,
          _eq1("fp_reduce_once", lambda s: s % P)),
        S("fp_reduce_2p", REDUCE_2P, False,
          carry_singles(rng, 4 * P, [0, P - 1, P, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P, 4 * P - 1]), _pack_fp,
          _eq1("fp_reduce_2p", lambda a: a - 2 * P if a >= 2 * P else a)),
        S("fp_canon3", CANON3, True,
          carry_singles(rng, 3 * P, [0, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P - 1]), _pack_fp,
          _eq1("fp_canon3", lambda x: x % P)),
        S("fp_mul", MUL, False, mul_pairs, _pack_fp, _check_mul("fp_mul", lazy=False)),
        S("fp_sqr", SQR, False, [(a,) for a in canon_vals], _pack_fp, _check_mul("fp_sqr", lazy=False)),
        S("fp_mul_lazy", MUL_LAZY, False, lazy_pairs, _pack_fp, _check_mul("fp_mul_lazy", lazy=True)),
        S("fp_sqr_d28_lazy", SQR_D28_LAZY, True, [(a,) for a in lazy_vals], _pack_fp,
          _check_mul("fp_sqr_d28_lazy", lazy=True)),
        S("fp2_mul_d28", FP2_MUL_D28, True, quads, _pack_fp, _check_fp2("fp2_mul_d28", _fp2_mul_ref)),
        S("fp2_sqr_d28", FP2_SQR_D28, True, sq_pairs, _pack_fp, _check_fp2("fp2_sqr_d28", _fp2_sqr_ref)),
        S("fp2_mul", FP2_MUL, True, quads, _pack_fp, _check_fp2("fp2_mul", _fp2_mul_ref)),
        S("fp2_sqr", FP2_SQR, True, sq_pairs, _pack_fp, _check_fp2("fp2_sqr", _fp2_sqr_ref)),
        S("fp2_mul_s", FP2_MUL_S, True, quads_s, _pack_fp, _check_fp2("fp2_mul_s", _fp2_mul_ref)),
        S("lz_mul_w", LZ_MUL_RAW, True, raw, lambda r: [d & 0xFFFFFFFF for d in r[0] + r[1]], _check_lz_raw(0)),
        S("lz_sqr_w", LZ_SQR_RAW, True, raw, lambda r: [d & 0xFFFFFFFF for d in r[0]], _check_lz_raw(1)),
        S("lz_fp_ops", LZ_FP_OPS, True, lz_fp_pairs(rng), pack_mont, _check_lz_fp),
        S("lz_fp2_ops", LZ_FP2_OPS, True, lz_fp2_pairs(rng), pack_mont2, _check_lz_fp2),
        S("fp_inv", INV, True, inv_vals, pack_mont, _check_inv("fp_inv", zero_ok=False)),
        S("fp_inv_gcd", INV_GCD, True, [(0,)] + inv_vals, pack_mont, _check_inv("fp_inv_gcd", zero_ok=True)),
        S("fp_sqrt", SQRT, True, sqrt_inputs(rng), pack_mont, _check_sqrt),
        S("fp2_inv", FP2_INV, True, fp2_inv_vals, pack_mont, _check_fp2_inv),
        S("fp2_sqrt", FP2_SQRT, True, fp2_sqrt_inputs(rng), pack_mont, _check_fp2_sqrt),
        S("coop_lin", LIN8, True, lin8_records(rng), _pack_lin8, _check_lin8),
        S("preds", PREDS, False, preds_records(rng), _pack_fp, _check_preds),
    ]


_SETS = None


def sets() -> dict:
    """name -> VectorSet, generated once per process"""
    global _SETS
    if _SETS is None:
        _SETS = {s.name: s for s in build_sets()}
    return _SETS


SET_NAMES = ("fp_add", "fp_sub", "fp_neg", "fp_dbl", "fp_half", "fp_add_nr", "fp_sub_nr", "fp_reduce_once",
             "fp_reduce_2p", "fp_canon3", "fp_mul", "fp_sqr", "fp_mul_lazy", "fp_sqr_d28_lazy", "fp2_mul_d28",
             "fp2_sqr_d28", "fp2_mul", "fp2_sqr", "fp2_mul_s", "lz_mul_w", "lz_sqr_w", "lz_fp_ops", "lz_fp2_ops",
             "fp_inv", "fp_inv_gcd", "fp_sqrt", "fp2_inv", "fp2_sqrt", "coop_lin", "preds")
D28_ONLY = frozenset(("fp_canon3", "fp_sqr_d28_lazy", "fp2_mul_d28", "fp2_sqr_d28", "fp2_mul", "fp2_sqr", "fp2_mul_s",
                      "lz_mul_w", "lz_sqr_w", "lz_fp_ops", "lz_fp2_ops", "fp_inv", "fp_inv_gcd", "fp_sqrt", "fp2_inv",
                      "fp2_sqrt", "coop_lin"))
# (set name, flavour) of every launch: the 32-bit column kernels where the op exists there
CASES = [(nm, fl) for nm in SET_NAMES for fl in ((D28,) if nm in D28_ONLY else (0, D28))]
