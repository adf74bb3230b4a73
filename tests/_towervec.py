"""Vectors and exact references of the device tower-op self-test
(include/lodestar_bls.h bls_gpu_tower_op_test, kernels/tower_ops.hpp, kernels/k_mlq.hip,
kernels/k_fin_simt.hip).

One TowerOp per op: its records, chosen on the RAW words (a raw coefficient p - 1 is the
stored Montgomery-form value; every raw coefficient lies in [0, p), because production never
passes anything else into these functions), the reference from oracle/bls_oracle.py alone,
and an exact check of the device's output words: every output Fp's raw value must be < p
(every producing function documents a canonical output) and its residue out of Montgomery
form must equal the reference.  A failure names op, translation unit, record and coefficient.

References.  O.f12_mul is schoolbook over w^6 = xi, independent of every Karatsuba
arrangement under test; every product op is the f12_mul of its operands embedded in Fp12
(an Fp6 at the even powers of w, a line (l0, l2, l3) as l0 + l2 w^2 + l3 w^3, fp6_mul_01's
(d0, d1) as d0 + d1 w^2, fp6_mul_1's d1 as d1 w^2).  The Frobenius maps are
conj(c_k) xi^(k(p-1)/6) and c_k xi^(k(p^2-1)/6) with the constants recomputed by f2_pow.
fp6_inv and fp12_inv are checked by f12_mul(a, got) == 1 (the inverse is unique, so this is
exact; 0 has none and is left out of the inversion records).  The cyclotomic ops only receive
members of the cyclotomic subgroup, as in production, and compare with plain f12_sqr and
conj(f12_pow(base, |x|)).  The line-buffer op compares with a restatement of
pairing.hpp's miller_dbl_step / miller_add_step and k_mlq.hip's store_line over the
oracle's Fp2 (ref_lines), which tests/test_towervec_cpu.py ties to O.miller_loop.

tests/test_gpu_tower_ops.py runs the ops on the GPU; tests/test_towervec_cpu.py proves the
references consistent, the edge records' raw patterns and which record reaches which
Karatsuba site's largest operand, and runs the header-function records through the CPU build."""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass
from typing import Callable

from oracle import bls_oracle as O
from tests import _curvevec as C
from tests._fieldvec import limbs, mont, unmont

P = O.P
D28 = 0x100  # BLS_TOWER_OP_D28
ONE = (1 << 384) % P  # Montgomery one, raw
H_LO, H_HI = (P - 1) // 2, (P + 1) // 2
XI = (1, 1)
N_RANDOM = 24

# base op ids (csrc/kernels/tower_op_ids.hpp TOP_*)
(FP6_MUL, FP6_MUL_01, FP6_MUL_1, FP6_INV, FP12_MUL, FP12_SQR, FP12_MUL_LINE, FP12_INV, FP12_FROB, FP12_FROB2,
 FIN_MUL12M, FIN_MUL12M_CONJ, FIN_CYC_SQR, FIN_EXP_X_M, MLQ_SQR12, MLQ_MUL_LINE12, MLQ_MUL_LINE2, MLQ_SQR12_PAIR,
 MLQ_MUL_LINE12_PAIR, MLQ_LINES) = range(20)
N_OPS = 20
TU = {0: "k_selftest (32-bit columns)", D28: "k_selftest_d28 (28-bit digits)"}
TU_FIN = "k_fin_simt (28-bit digits)"
TU_MLQ = "k_mlq (28-bit digits + Fp2 primitive)"

# operand kinds: Fp2 values per operand, in memory order
KIND_N2 = {"f12": 6, "f6": 3, "line": 3, "d01": 2, "d1": 1}
_F12_ORDER = C._F12_ORDER  # memory position n holds the coefficient of w^_F12_ORDER[n]


def neg(v: int) -> int:
    return (P - v) % P


# ---- raw operands <-> oracle elements ------------------------------------------------------------
def element(kind: str, raw) -> list:
    """the Fp12 element (6 coefficients of w^k) a raw operand stands for"""
    vals = [unmont(v) for v in raw]
    f2s = [(vals[2 * k], vals[2 * k + 1]) for k in range(len(vals) // 2)]
    z = O.F2_ZERO
    if kind == "f12":
        return C.f12_unpack(vals)
    if kind == "f6":
        return [f2s[0], z, f2s[1], z, f2s[2], z]
    if kind == "line":
        return [f2s[0], z, f2s[1], f2s[2], z, z]
    if kind == "d01":
        return [f2s[0], z, f2s[1], z, z, z]
    return [z, z, f2s[0], z, z, z]  # d1


def raw_f12(f) -> tuple:
    """oracle Fp12 element -> raw operand (memory order, Montgomery form)"""
    return tuple(mont(c) for k in _F12_ORDER for c in f[k])


def pack(operands) -> list[int]:
    return [w for raw in operands for v in raw for w in limbs(v)]


F6_NAMES = tuple(f"c{k}.c{j}" for k in (0, 1, 2) for j in (0, 1))
F12_NAMES = tuple(n[2:] for n in C.F12_NAMES)


def out_element(kind: str, words, at: int = 0):
    """(Fp12 element, None) of the Fp6 / Fp12 at Fp index `at` of the output words, or (None,
    the description of the first Fp that is not canonical)"""
    names = F6_NAMES if kind == "f6" else F12_NAMES
    vals, err = C.fps_out(words, names, at=12 * at)
    if err:
        return None, err
    return element(kind, [mont(v) for v in vals]), None


def cmp_element(kind: str, got, want):
    order = (0, 2, 4) if kind == "f6" else _F12_ORDER
    names = F6_NAMES if kind == "f6" else F12_NAMES
    if kind == "f6":
        assert all(want[k] == O.F2_ZERO for k in (1, 3, 5)), "the reference left Fp6"
    for n, k in enumerate(order):
        for j in (0, 1):
            if got[k][j] != want[k][j]:
                return f"{names[2 * n + j]} = {got[k][j]:#x}, want {want[k][j]:#x} (plain residues)"


# ---- edge operands -----------------------------------------------------------------------------------
COMMON = ("p-1", "zero", "one", "alt a", "alt b", "c0s p-1", "c1s p-1", "half-", "half+")
# "c0s p-1" / "c1s p-1": every Fp2 (p-1, 0) resp. (0, p-1).  The Fp2 product's c0 is
# a0 b0 - a1 b1 (the rows add an offset of 4.00003 p^2 so that no column goes negative): sums of
# such operands are (2p-2, 0) and (0, 2p-2), the two ends of that difference at the sites'
# bound.  In the alternating patterns and in all-p-1 the two halves of every sum are equal and
# the difference cancels.


def _rand_raw(rng, n2):
    return tuple(rng.randrange(P) for _ in range(2 * n2))


def _nz(rng):
    return rng.randrange(1, P)


def edge_operands(kind: str, rng) -> list:
    """(pattern name, raw operand): the raw patterns of one operand"""
    n2 = KIND_N2[kind]
    alt = [(P - 1, 0), (0, P - 1)]
    E = [("p-1", (P - 1,) * (2 * n2)), ("zero", (0,) * (2 * n2)), ("one", (ONE,) + (0,) * (2 * n2 - 1)),
         ("alt a", tuple(v for k in range(n2) for v in alt[k % 2])),
         ("alt b", tuple(v for k in range(n2) for v in alt[(k + 1) % 2])),
         ("c0s p-1", (P - 1, 0) * n2), ("c1s p-1", (0, P - 1) * n2),
         ("half-", (H_LO,) * (2 * n2)), ("half+", (H_HI,) * (2 * n2))]
    r = list(_rand_raw(rng, n2))
    if kind == "f12":    # a.c1 = -a.c0: fp6_add(a.c0, a.c1) = 0
        E.append(("neg", tuple(r[:6] + [neg(v) for v in r[:6]])))
    elif kind == "f6":   # a.c1 = -a.c0 in Fp2: the unreduced sum a.c0 + a.c1 is exactly p
        E.append(("neg", tuple(r[:2] + [neg(v) for v in r[:2]] + r[4:])))
    elif kind == "line":  # l2 = -l3
        E.append(("neg", tuple(r[:2] + [neg(v) for v in r[4:]] + r[4:])))
    elif kind == "d01":
        E.append(("neg", tuple(r[:2] + [neg(v) for v in r[:2]])))
    E.append(("only c0.c0", (_nz(rng),) + (0,) * (2 * n2 - 1)))
    if kind == "f12":
        E.append(("only c0", tuple(_nz(rng) for _ in range(6)) + (0,) * 6))
        E.append(("only c1", (0,) * 6 + tuple(_nz(rng) for _ in range(6))))
    for k in range(n2):
        E.append((f"only Fp2 {k}", tuple(_nz(rng) if j // 2 == k else 0 for j in range(2 * n2))))
    if kind == "line":
        for k, nm in enumerate(("l0 = 0", "l2 = 0", "l3 = 0")):
            E.append((nm, tuple(0 if j // 2 == k else _nz(rng) for j in range(6))))
    return E


def has_pattern(kind: str, name: str, raw) -> bool:
    """whether a raw operand really has the pattern its record is named for"""
    n2 = KIND_N2[kind]
    raw = list(raw)
    f2 = [tuple(raw[2 * k: 2 * k + 2]) for k in range(n2)]
    if not (len(raw) == 2 * n2 and all(0 <= v < P for v in raw)):
        return False
    if name == "p-1":
        return all(v == P - 1 for v in raw)
    if name == "zero":
        return not any(raw)
    if name == "one":
        return raw[0] == ONE and not any(raw[1:]) and unmont(raw[0]) == 1
    if name in ("alt a", "alt b"):
        ph = 0 if name == "alt a" else 1
        return all(f2[k] == ((P - 1, 0) if (k + ph) % 2 == 0 else (0, P - 1)) for k in range(n2))
    if name in ("c0s p-1", "c1s p-1"):
        return all(c == ((P - 1, 0) if name == "c0s p-1" else (0, P - 1)) for c in f2)
    if name == "half-":
        return all(v == H_LO for v in raw) and 2 * H_LO == P - 1
    if name == "half+":
        return all(v == H_HI for v in raw) and 2 * H_HI == P + 1
    if name == "neg":
        if kind == "f12":
            return all((raw[j] + raw[6 + j]) % P == 0 for j in range(6)) and any(raw[:6])
        if kind == "line":
            return all((raw[2 + j] + raw[4 + j]) % P == 0 for j in range(2)) and any(raw[2:4])
        return all((raw[j] + raw[2 + j]) % P == 0 for j in range(2)) and any(raw[:2])
    if name == "only c0.c0":
        return raw[0] != 0 and not any(raw[1:])
    if name == "only c0":
        return all(raw[:6]) and not any(raw[6:])
    if name == "only c1":
        return all(raw[6:]) and not any(raw[:6])
    if name.startswith("only Fp2 "):
        k = int(name[9:])
        return all(f2[k]) and not any(v for j, v in enumerate(raw) if j // 2 != k)
    if name in ("l0 = 0", "l2 = 0", "l3 = 0"):
        k = ("l0 = 0", "l2 = 0", "l3 = 0").index(name)
        return f2[k] == (0, 0) and all(v for j, v in enumerate(raw) if j // 2 != k)
    return False


@dataclass(frozen=True)
class Record:
    label: str
    operands: tuple      # one raw operand (tuple of raw ints) per kind
    tags: tuple = ()     # (operand index, pattern name) of the operands that are not random


def product_records(kinds: tuple, seed: int, invertible: bool = False, extra=()) -> list:
    """each operand at each of its edge patterns with the others random; every operand at each
    common pattern; the extra records; N_RANDOM random ones"""
    rng = random.Random(seed)
    recs = []
    for j, kind in enumerate(kinds):
        for nm, raw in edge_operands(kind, rng):
            ops = tuple(raw if i == j else _rand_raw(rng, KIND_N2[k]) for i, k in enumerate(kinds))
            recs.append(Record(f"operand {j} ({kind}) {nm}, the others random", ops, ((j, nm),)))
    if len(kinds) > 1:
        for nm in COMMON:
            ops = tuple(dict(edge_operands(k, rng))[nm] for k in kinds)
            recs.append(Record(f"every operand {nm}", ops, tuple((j, nm) for j in range(len(kinds)))))
    recs += list(extra)
    recs += [Record(f"random {i}", tuple(_rand_raw(rng, KIND_N2[k]) for k in kinds)) for i in range(N_RANDOM)]
    if invertible:
        recs = [r for r in recs if any(r.operands[0])]
    return recs


def _conj_raw(raw):
    """conj of a raw Fp12 operand: c1 negated"""
    return tuple(raw[:6]) + tuple(neg(v) for v in raw[6:])


def _mul_extra(seed, conj_second: bool):
    rng = random.Random(seed)
    a = _rand_raw(rng, 6)
    p1 = (P - 1,) * 12
    ex = [Record("b = conj(a), a random", (a, _conj_raw(a))), Record("b = conj(a), a all p-1", (p1, _conj_raw(p1)))]
    if conj_second:
        # mul12m<true> adds m.c0 and -m.c1: with m.c1 = (p+1)/2 every coefficient of that sum is p - 1
        ex.append(Record("inner max: a half-, m = (half-, half+)", ((H_LO,) * 12, (H_LO,) * 6 + (H_HI,) * 6)))
    return ex


# f.c0 + f.c1 = l2 + l3 = p - 1 in every coefficient, l0 = p - 1: the second fp6_mul_01 of the line
# product gets raw p - 1 operands (with all-p-1 inputs these reduced sums are p - 2)
LINE_INNER_MAX = Record("inner max: f half-, l0 = p-1, l2 = l3 = half-", ((H_LO,) * 12, (P - 1,) * 2 + (H_LO,) * 4))


def _line2_extra(seed):
    rng = random.Random(seed)
    ex = []
    for nm, raw in edge_operands("line", rng):
        ex.append(Record(f"both lines {nm}, f random", (_rand_raw(rng, 6), raw, raw), ((1, nm), (2, nm))))
    ln = _rand_raw(rng, 3)
    ex.append(Record("the two lines equal (random), f random", (_rand_raw(rng, 6), ln, ln)))
    return ex


# ---- references -----------------------------------------------------------------------------------------
def f12_prod(els):
    acc = els[0]
    for e in els[1:]:
        acc = O.f12_mul(acc, e)
    return acc


@functools.lru_cache(maxsize=None)
def frob_consts():
    """(xi^(k(p-1)/6), xi^(k(p^2-1)/6)) for k = 0..5, recomputed"""
    return (tuple(O.f2_pow(XI, k * (P - 1) // 6) for k in range(6)),
            tuple(O.f2_pow(XI, k * (P * P - 1) // 6) for k in range(6)))


def ref_frob(a):
    return [O.f2_mul(O.f2_conj(c), frob_consts()[0][k]) for k, c in enumerate(a)]


def ref_frob2(a):
    return [O.f2_mul(c, frob_consts()[1][k]) for k, c in enumerate(a)]


def ref_exp_x(a):
    return O.f12_conj(O.f12_pow(a, O.X_ABS))


@functools.lru_cache(maxsize=None)
def cyclotomic_inputs():
    """(name, element of the cyclotomic subgroup): 1, (conj f / f)^(p^2 + 1) of random f, an
    r-th power of one of them, a value of order r from the oracle's pairing"""
    rng = random.Random(0xC7C10)

    def easy(f):
        t = O.f12_mul(O.f12_conj(f), O.f12_inv(f))
        return O.f12_mul(ref_frob2(t), t)

    cs = [easy([(rng.randrange(P), rng.randrange(P)) for _ in range(6)]) for _ in range(8)]
    recs = [("one", list(O.F12_ONE))]
    recs += [(f"(conj f / f)^(p^2 + 1), random f {k}", c) for k, c in enumerate(cs)]
    recs.append(("an r-th power", O.f12_pow(cs[0], O.R)))
    recs.append(("of order r: e(g1, g2)", O.pairing(O.G1, O.G2)))
    return tuple((nm, tuple(c)) for nm, c in recs)


def cyclotomic_records() -> list:
    return [Record(nm, (raw_f12(c),)) for nm, c in cyclotomic_inputs()]


# ---- the line buffer ----------------------------------------------------------------------------------------
LINE_EVENTS = 68
_INV2 = pow(2, -1, P)


def _half(a):
    return O.f2_muls(a, _INV2)


def _dbl(a):
    return O.f2_add(a, a)


def _dbl_step(T):
    """pairing.hpp miller_dbl_step"""
    x, y, z = T
    a = _half(O.f2_mul(x, y))
    b = O.f2_sqr(y)
    c = O.f2_sqr(z)
    c3 = O.f2_add(_dbl(c), c)
    e = O.f2_mul(XI, _dbl(_dbl(c3)))
    f = O.f2_add(_dbl(e), e)
    g = _half(O.f2_add(b, f))
    h = O.f2_sub(O.f2_sqr(O.f2_add(y, z)), O.f2_add(b, c))
    i = O.f2_sub(e, b)
    j = O.f2_sqr(x)
    e2 = O.f2_sqr(e)
    T2 = (O.f2_mul(a, O.f2_sub(b, f)), O.f2_sub(O.f2_sqr(g), O.f2_add(_dbl(e2), e2)), O.f2_mul(b, h))
    return T2, (i, O.f2_add(_dbl(j), j), O.f2_neg(h))


def _add_step(T, Q):
    """pairing.hpp miller_add_step"""
    x, y, z = T
    theta = O.f2_sub(y, O.f2_mul(Q[1], z))
    lam = O.f2_sub(x, O.f2_mul(Q[0], z))
    c = O.f2_sqr(theta)
    d = O.f2_sqr(lam)
    e = O.f2_mul(lam, d)
    f = O.f2_mul(z, c)
    g = O.f2_mul(x, d)
    h = O.f2_sub(O.f2_add(e, f), _dbl(g))
    T2 = (O.f2_mul(lam, h), O.f2_sub(O.f2_mul(theta, O.f2_sub(g, h)), O.f2_mul(e, y)), O.f2_mul(z, e))
    return T2, (O.f2_sub(O.f2_mul(theta, Q[0]), O.f2_mul(lam, Q[1])), O.f2_neg(theta), lam)


def line_event_names() -> list[str]:
    names = []
    for bit in range(62, -1, -1):
        names.append(f"doubling at bit {bit}")
        if (O.X_ABS >> bit) & 1:
            names.append(f"addition at bit {bit}")
    return names


@functools.lru_cache(maxsize=None)
def ref_lines(pa, q) -> tuple:
    """the 68 lines (l0, l2, l3) k_mlq writes for P = pa (affine), Q = q: each step's (c0, c1,
    c2) scaled as store_line does, l0 = c0, l2 = c1 x_P, l3 = c2 y_P"""
    T = (q[0], q[1], O.F2_ONE)
    out = []
    for bit in range(62, -1, -1):
        T, c = _dbl_step(T)
        out.append((c[0], O.f2_muls(c[1], pa[0]), O.f2_muls(c[2], pa[1])))
        if (O.X_ABS >> bit) & 1:
            T, c = _add_step(T, q)
            out.append((c[0], O.f2_muls(c[1], pa[0]), O.f2_muls(c[2], pa[1])))
    assert len(out) == LINE_EVENTS
    return tuple(out)


def lines_to_f(lines):
    """the lines multiplied in kernels/k_mlq.hip ml_f's order (one squaring per bit), conjugated"""
    f = list(O.F12_ONE)
    e = 0
    z = O.F2_ZERO
    for bit in range(62, -1, -1):
        if bit != 62:
            f = O.f12_sqr(f)
        for _ in range(1 + ((O.X_ABS >> bit) & 1)):
            l0, l2, l3 = lines[e]
            f = O.f12_mul(f, [l0, z, l2, l3, z, z])
            e += 1
    return O.f12_conj(f)


def line_items():
    """(P affine, Jacobian z, Q): six items of tests/_curvevec.py's Miller set -- z random at
    0, 2, 3, 5 (g1_eval_affine_from_jac inverts it), z = 1 at 1, 4"""
    return tuple((pa, z, q) for pa, z, q, _d in C.miller_items()[:6])


def pack_line_item(item) -> list[int]:
    (x, y), z, q = item
    return C.pack_fps([x * z * z % P, y * z * z * z % P, z]) + C.pack_fps(C._flat(q))


LINE_FP_NAMES = tuple(f"{l}.c{j}" for l in ("l0", "l2", "l3") for j in (0, 1))


def check_lines(item, words):
    pa, _z, q = item
    want = ref_lines(pa, q)
    ev = line_event_names()
    for e in range(LINE_EVENTS):
        names = tuple(f"line {e} ({ev[e]}) {n}" for n in LINE_FP_NAMES)
        got, err = C.fps_out(words, names, at=72 * e)
        err = err or C._cmp(names, got, [c for l in want[e] for c in l])
        if err:
            return err


# ---- the ops -------------------------------------------------------------------------------------------------
@dataclass
class TowerOp:
    name: str
    op: int
    flavours: tuple      # 0: the 32-bit column product, D28: the 28-bit-digit one
    tu: str | None       # fixed translation unit (k_fin_simt / k_mlq), else by flavour
    kinds: tuple         # operand kinds
    out: str             # "f6", "f12" or "pair" (two Fp12: lane 2k's, lane 2k + 1's)
    ref: Callable | None  # operand elements -> Fp12 element; None: an inversion
    make: Callable       # () -> list of Record

    def where(self, flavour: int) -> str:
        return self.tu or TU[flavour]

    @functools.cached_property
    def records(self) -> list:
        return self.make()

    def check(self, rec: Record, words):
        """None, or what is wrong with the output words of `rec`"""
        els = [element(k, raw) for k, raw in zip(self.kinds, rec.operands)]
        kind = "f6" if self.out == "f6" else "f12"
        for lane in range(2 if self.out == "pair" else 1):
            pre = f"lane 2k + {lane}: " if self.out == "pair" else ""
            got, err = out_element(kind, words, at=12 * lane)
            if err:
                return pre + err
            if self.ref is None:
                prod = O.f12_mul(els[0], got)
                err = cmp_element("f12", prod, list(O.F12_ONE))
                err = err and "a * result != 1: " + err + f"; result {C.hx(got)}"
            else:
                err = cmp_element(kind, got, ref_cache(self, rec, els))
            if err:
                return pre + err


_REF = {}


def ref_cache(op: TowerOp, rec: Record, els):
    """the reference of (op's function, operands), computed once per module"""
    key = (op.ref, rec.operands)
    if key not in _REF:
        _REF[key] = op.ref(els)
    return _REF[key]


def _sqr(els):
    return O.f12_sqr(els[0])


def _mul_conj(els):
    return O.f12_mul(els[0], O.f12_conj(els[1]))


def _ops():
    T = TowerOp
    PR = product_records
    f12_1 = functools.lru_cache(maxsize=None)(lambda: PR(("f12",), 0x5012))
    f12_inv = lambda: PR(("f12",), 0x1012, invertible=True)  # noqa: E731
    f12_2 = functools.lru_cache(maxsize=None)(lambda: PR(("f12", "f12"), 0x2012, extra=_mul_extra(0x2013, False)))
    f12_2c = lambda: PR(("f12", "f12"), 0x2014, extra=_mul_extra(0x2015, True))  # noqa: E731
    f12_line = functools.lru_cache(maxsize=None)(lambda: PR(("f12", "line"), 0x3012, extra=[LINE_INNER_MAX]))
    f12_line2 = lambda: PR(("f12", "line", "line"), 0x4012, extra=_line2_extra(0x4013))  # noqa: E731
    cyc = functools.lru_cache(maxsize=None)(cyclotomic_records)
    return [
        T("fp6_mul", FP6_MUL, (0, D28), None, ("f6", "f6"), "f6", f12_prod, lambda: PR(("f6", "f6"), 0x6012)),
        T("fp6_mul_01", FP6_MUL_01, (0,), None, ("f6", "d01"), "f6", f12_prod, lambda: PR(("f6", "d01"), 0x6013)),
        T("fp6_mul_1", FP6_MUL_1, (0,), None, ("f6", "d1"), "f6", f12_prod, lambda: PR(("f6", "d1"), 0x6014)),
        T("fp6_inv", FP6_INV, (D28,), None, ("f6",), "f6", None, lambda: PR(("f6",), 0x6015, invertible=True)),
        T("fp12_mul", FP12_MUL, (0,), None, ("f12", "f12"), "f12", f12_prod, f12_2),
        T("fp12_sqr", FP12_SQR, (0,), None, ("f12",), "f12", _sqr, f12_1),
        T("fp12_mul_line", FP12_MUL_LINE, (0,), None, ("f12", "line"), "f12", f12_prod, f12_line),
        T("fp12_inv", FP12_INV, (D28,), None, ("f12",), "f12", None, f12_inv),
        T("fp12_frob", FP12_FROB, (D28,), None, ("f12",), "f12", lambda e: ref_frob(e[0]), f12_1),
        T("fp12_frob2", FP12_FROB2, (D28,), None, ("f12",), "f12", lambda e: ref_frob2(e[0]), f12_1),
        T("mul12m", FIN_MUL12M, (D28,), TU_FIN, ("f12", "f12"), "f12", f12_prod, f12_2),
        T("mul12m_conj", FIN_MUL12M_CONJ, (D28,), TU_FIN, ("f12", "f12"), "f12", _mul_conj, f12_2c),
        T("cyc_sqr", FIN_CYC_SQR, (D28,), TU_FIN, ("f12",), "f12", _sqr, cyc),
        T("exp_x_m", FIN_EXP_X_M, (D28,), TU_FIN, ("f12",), "f12", lambda e: ref_exp_x(e[0]), cyc),
        T("sqr12", MLQ_SQR12, (D28,), TU_MLQ, ("f12",), "f12", _sqr, f12_1),
        T("mul_line12", MLQ_MUL_LINE12, (D28,), TU_MLQ, ("f12", "line"), "f12", f12_prod, f12_line),
        T("fp12_mul_line2", MLQ_MUL_LINE2, (D28,), TU_MLQ, ("f12", "line", "line"), "f12", f12_prod, f12_line2),
        T("sqr12_pair", MLQ_SQR12_PAIR, (D28,), TU_MLQ, ("f12",), "pair", _sqr, f12_1),
        T("mul_line12_pair", MLQ_MUL_LINE12_PAIR, (D28,), TU_MLQ, ("f12", "line"), "pair", f12_prod, f12_line),
    ]


OPS = {t.name: t for t in _ops()}
FLAVOUR_ID = {0: "cols", D28: "d28"}
CASES = [(t.name, fl) for t in OPS.values() for fl in t.flavours]
CASE_IDS = [f"{nm}-{'fin' if OPS[nm].tu == TU_FIN else 'mlq' if OPS[nm].tu == TU_MLQ else FLAVOUR_ID[fl]}" for nm, fl in CASES]
# fp12_cyclotomic_sqr and fp12_cyclotomic_exp_x have no device op: no production kernel
# compiles them (k_fin_simt.hip runs its own cyc_sqr / exp_x_m); tests/test_towervec_cpu.py
# runs the cyclotomic records through their CPU build


def failure(t: TowerOp, flavour: int, i: int, rec: Record, err: str) -> str:
    return f"{t.name} in {t.where(flavour)}, record {i} [{rec.label}]: {err}"


# ---- the unreduced Karatsuba sums, on raw integers --------------------------------------------------------
def _f2s(raw):
    return [tuple(raw[2 * k: 2 * k + 2]) for k in range(len(raw) // 2)]


def _add(a, b):      # fp2_add on raw Montgomery values (the form is linear)
    return tuple((x + y) % P for x, y in zip(a, b))


def _add_nr(a, b):   # fp2_add_nr
    return tuple(x + y for x, y in zip(a, b))


def sites_fp6_mul(a, b, pre=""):
    """site -> the largest coefficient fp2_mul_s receives there (a, b: three raw Fp2 each)"""
    out = {}
    for nm, (i, j) in (("c0", (1, 2)), ("c1", (0, 1)), ("c2", (0, 2))):
        out[f"{pre}fp6_mul {nm}"] = max(_add_nr(a[i], a[j]) + _add_nr(b[i], b[j]))
    return out


def sites_fp6_mul_01(a, d0, d1, pre=""):
    return {f"{pre}fp6_mul_01 c1": max(_add_nr(a[0], a[1]) + _add_nr(d0, d1))}


def sites_fp12_mul(a, b, conj=False):
    """fp12_mul / mul12m<conj>: the three fp6_mul calls"""
    a, b = _f2s(a), _f2s(b)
    bc1 = [tuple(neg(v) for v in c) for c in b[3:]] if conj else b[3:]
    out = sites_fp6_mul(a[:3], b[:3], "t0: ")
    out.update(sites_fp6_mul(a[3:], b[3:], "t1: "))
    out.update(sites_fp6_mul([_add(x, y) for x, y in zip(a[:3], a[3:])], [_add(x, y) for x, y in zip(b[:3], bc1)],
                             "(a.c0 + a.c1)(b.c0 + b.c1): "))
    return out


def sites_mul_line(f, line):
    """fp12_mul_line / mul_line12: the two fp6_mul_01 calls"""
    f, (l0, l2, l3) = _f2s(f), _f2s(line)
    out = sites_fp6_mul_01(f[:3], l0, l2, "aa: ")
    out.update(sites_fp6_mul_01([_add(x, y) for x, y in zip(f[:3], f[3:])], l0, _add(l2, l3), "(f.c0 + f.c1): "))
    return out


def sites_line2_lines(l, m):
    """fp12_mul_line2: the three products of the two lines' sums"""
    (l0, l2, l3), (m0, m2, m3) = _f2s(l), _f2s(m)
    return {"a2": max(_add_nr(l0, l2) + _add_nr(m0, m2)), "a3": max(_add_nr(l0, l3) + _add_nr(m0, m3)),
            "a5": max(_add_nr(l2, l3) + _add_nr(m2, m3))}
