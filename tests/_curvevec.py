"""Vectors and exact references of the device curve-op self-test
(include/lodestar_bls.h bls_gpu_curve_op_test, kernels/curve_ops.hpp, kernels/k_chain.hip).

One VectorSet per op: its records (Python integers, oracle points), how a record packs into
32-bit words (Fp = 12 little-endian words of the Montgomery form), the reference from
oracle/bls_oracle.py alone, and a check of the device's output words against it -- exact:
every Fp word group is taken out of Montgomery form and compared as a residue, and the raw
value must be canonical (< p), which is what every producing function documents in
bls/field.hpp for these flavours (fp_add / fp_sub / fp_neg / fp_half reduce; fp_mul and
fp_sqr without LAZY are "canonical"; fp2_mul / fp2_sqr and the out-of-line Fp2 primitive
are "canonical out").  Jacobian outputs compare as the affine point.  A failure names the
op, the flavour's translation unit, the record and the coordinate.

The inputs are the ones no message reaches through SHA-256: u = 0, u on the axes, the u
whose g(x1) lies in Fp (the fast map's refusal, fp2_sqrt's a1 == 0 case), the poles of the
isogeny, infinity and small-order points into the cofactor clearing, and q1 = +-q0 / poles
into k_chain's role 0.

tests/test_gpu_curve_ops.py runs the sets on the GPU; tests/test_curvevec_cpu.py proves the
references consistent and runs the same records through the CPU build of the same headers."""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass
from typing import Callable

from oracle import bls_oracle as O
from tests import _groupedge as ge
from tests._fieldvec import limbs, mont, unlimbs, unmont

P = O.P
D28 = 0x100  # BLS_CURVE_OP_D28

# base op ids (csrc/kernels/curve_op_ids.hpp COP_*)
FROM_BE64, H2F, SSWU, SSWU_FAST, ISO_AFF, ISO_JAC, CLEAR_COFACTOR, CHAIN_H = range(8)
N_OPS = 8
# the translation unit an (op, flavour) runs in, for failure messages
TU = {0: "k_selftest (32-bit columns)", D28: "k_selftest_d28 (28-bit digits)"}
TU_CHAIN = "k_chain (28-bit digits + Fp2 primitive)"

N_RANDOM_U = 200


def hx(v) -> str:
    if v is None:
        return "O"
    return "(" + ", ".join(hx(c) for c in v) + ")" if isinstance(v, (tuple, list)) else hex(v)


# ---- packing and unpacking ----------------------------------------------------------------
def pack_fps(vals) -> list[int]:
    """plain residues -> Montgomery-form words"""
    return [w for v in vals for w in limbs(mont(v))]


def pack_f2s(*f2s) -> list[int]:
    return pack_fps([c for a in f2s for c in a])


def raw_fps(words, n, at=0) -> list[int]:
    return [unlimbs(words[at + 12 * k: at + 12 * k + 12]) for k in range(n)]


def fps_out(words, names, at=0):
    """(plain residues, None) of the len(names) Fp values at word `at`, or (None, the
    description of the first one that is not canonical)"""
    raw = raw_fps(words, len(names), at)
    for nm, v in zip(names, raw):
        if v >= P:
            return None, f"{nm} = {v:#x} is not canonical (>= p)"
    return [unmont(v) for v in raw], None


XY = ("x.c0", "x.c1", "y.c0", "y.c1")


def _cmp(names, got, want):
    for nm, g, w in zip(names, got, want):
        if g != w:
            return f"{nm} = {g:#x}, want {w:#x} (plain residues)"


def _flat(pt):
    return [pt[0][0], pt[0][1], pt[1][0], pt[1][1]]


# ---- FROM_BE64 -------------------------------------------------------------------------------
def from_be64_values() -> list[int]:
    rng = random.Random(0xBE64)
    top = 1 << 512
    q = top // P * P
    vals = [0, 1, P - 1, P, P + 1, (1 << 256) - 1, ((1 << 256) - 1) << 256, 1 << 256, top - 1, q, q - 1, q + 1]
    vals += [rng.randrange(top) for _ in range(32)]
    assert all(0 <= v < top for v in vals)
    return vals


def pack_be64(v: int) -> list[int]:
    return [(v >> (32 * (15 - k))) & 0xFFFFFFFF for k in range(16)]  # most significant word first


def check_from_be64(v, out):
    got, err = fps_out(out, ("value",))
    return err or _cmp(("value",), got, [v % P])


# ---- H2F ---------------------------------------------------------------------------------------
def h2f_messages() -> list[bytes]:
    rng = random.Random(0x42F)
    msgs = [bytes(32), b"\xff" * 32]
    for k in range(8):  # one set bit in each of the 8 words
        m = bytearray(32)
        bit = (5 * k + 3) % 32
        m[4 * k + 3 - bit // 8] = 1 << (bit % 8)
        msgs.append(bytes(m))
    msgs += [rng.randbytes(32) for _ in range(64)]
    return msgs


def pack_msg(m: bytes) -> list[int]:
    return [int.from_bytes(m[4 * k: 4 * k + 4], "big") for k in range(8)]


U01 = ("u0.c0", "u0.c1", "u1.c0", "u1.c1")


def ref_h2f(m: bytes):
    u0, u1 = O.hash_to_field_fp2(m, 2, O.DST_POP)
    return [u0[0], u0[1], u1[0], u1[1]]


def check_h2f(m, out):
    got, err = fps_out(out, U01)
    return err or _cmp(U01, got, ref_h2f(m))


# ---- SSWU ----------------------------------------------------------------------------------------
def g_iso(x):
    """g(x) = x^3 + A' x + B' of E2'"""
    return O.f2_add(O.f2_add(O.f2_mul(O.f2_sqr(x), x), O.f2_mul(O.A_ISO, x)), O.B_ISO)


def sswu_x1(u):
    """(den, x1) of RFC 9380 6.6.2 for u (den == 0: the exceptional x1)"""
    zu2 = O.f2_mul(O.Z_SSWU, O.f2_sqr(u))
    den = O.f2_add(O.f2_sqr(zu2), zu2)
    if O.f2_is_zero(den):
        return den, O.f2_mul(O.B_ISO, O.f2_inv(O.f2_mul(O.Z_SSWU, O.A_ISO)))
    return den, O.f2_mul(O.f2_mul(O.f2_neg(O.B_ISO), O.f2_inv(O.A_ISO)), O.f2_add(O.F2_ONE, O.f2_inv(den)))


def sswu_gx(u):
    """(den, g(x1) is a square, the g(x) of the x the map takes)"""
    den, x1 = sswu_x1(u)
    g1 = g_iso(x1)
    if O.f2_is_square(g1):
        return den, True, g1
    return den, False, g_iso(O.f2_mul(O.f2_mul(O.Z_SSWU, O.f2_sqr(u)), x1))


def fast_ok(u) -> bool:
    """what map_to_curve_sswu_fast must return: false for den == 0 and for g(x).c1 == 0"""
    den, _sq, g = sswu_gx(u)
    return not O.f2_is_zero(den) and g[1] != 0


@functools.lru_cache(maxsize=None)
def c1_zero_us():
    """u with g(x1).c1 == 0, as (u, g(x1).c0 is a square in Fp): x1 = (a, b) on
    3 a^2 b - b^3 + 240 a + 1012 = 0 for b = 0, 1, ..., each x1 pulled back through
    x1(u) = (-B/A)(1 + 1/den), den = t^2 + t, t = Z u^2 (every square root that exists).
    g(x1) then lies in Fp, so it is a square in Fp2 whatever its Legendre symbol: the map
    keeps x1, and its root is real (c0 a square in Fp) or purely imaginary (not)."""
    out = []
    inv2 = pow(2, -1, P)
    for b in range(60):
        if b == 0:
            cand = [-1012 * pow(240, -1, P) % P]
        else:
            s = O.fp_sqrt((240 * 240 - 12 * b * (1012 - b ** 3)) % P)
            if s is None:
                continue
            cand = [(-240 + s) * pow(6 * b, -1, P) % P, (-240 - s) * pow(6 * b, -1, P) % P]
        for a in cand:
            x1 = (a, b)
            g = g_iso(x1)
            assert g[1] == 0
            w = O.f2_sub(O.f2_mul(x1, O.f2_mul(O.f2_neg(O.A_ISO), O.f2_inv(O.B_ISO))), O.F2_ONE)  # 1 / den
            if O.f2_is_zero(w):
                continue
            s = O.f2_sqrt(O.f2_add(O.F2_ONE, O.f2_muls(O.f2_inv(w), 4)))
            if s is None:
                continue
            for sg in (s, O.f2_neg(s)):
                t = O.f2_muls(O.f2_sub(sg, O.F2_ONE), inv2)
                u = O.f2_sqrt(O.f2_mul(t, O.f2_inv(O.Z_SSWU)))
                if u is not None and sswu_x1(u)[1] == x1:
                    out.append((u, O.legendre(g[0]) == 1))
    return tuple(out)


def c1_zero_pick(per_kind: int = 5):
    """the first `per_kind` u of each kind (g(x1) a square in Fp / not)"""
    us = c1_zero_us()
    return [u for u, k in us if k][:per_kind] + [u for u, k in us if not k][:per_kind]


@functools.lru_cache(maxsize=None)
def sswu_inputs():
    """(directed u, each followed by -u; the random u)"""
    edge = [(0, 0)]
    for v in (1, 2, P - 1, P - 2):
        edge += [(v, 0), (0, v)]
    edge.append((P - 1, P - 1))
    edge += c1_zero_pick()
    directed = []
    for u in edge:
        directed.append(u)
        if u != (0, 0):
            directed.append(O.f2_neg(u))
    rng = random.Random(0x55C0)
    rand = [(rng.randrange(P), rng.randrange(P)) for _ in range(N_RANDOM_U)]
    return tuple(directed), tuple(rand)


def sswu_us():
    d, r = sswu_inputs()
    return list(d) + list(r)


@functools.lru_cache(maxsize=None)
def ref_sswu(u):
    return O.map_to_curve_sswu(u)


def check_sswu(u, out):
    got, err = fps_out(out, XY)
    return err or _cmp(XY, got, _flat(ref_sswu(u)))


def check_sswu_fast(u, out):
    want_ok = fast_ok(u)
    if out[0] != int(want_ok):
        return f"ok = {out[0]}, want {int(want_ok)}"
    if want_ok:
        got, err = fps_out(out, XY, at=1)
        return err or _cmp(XY, got, _flat(ref_sswu(u)))


# ---- the isogeny --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def iso_poles():
    """the distinct x at which iso_map has a pole: the roots of the x-denominator and of the
    y-denominator in Fp2.  (There is one: the x-denominator is (x - r)^2 and the
    y-denominator (x - r)^3, r the x of the dual isogeny's kernel;
    tests/test_curvevec_cpu.py proves it.)"""
    c0, c1 = O.ISO_XDEN[0], O.ISO_XDEN[1]
    s = O.f2_sqrt(O.f2_sub(O.f2_sqr(c1), O.f2_muls(c0, 4)))
    assert s is not None  # both roots of the x-denominator exist in Fp2
    inv2 = pow(2, -1, P)
    r1, r2 = (O.f2_muls(O.f2_sub(t, c1), inv2) for t in (s, O.f2_neg(s)))
    # yden = (x^2 + c1 x + c0)(x - r3): compare the x^2 coefficients
    r3 = O.f2_sub(c1, O.ISO_YDEN[2])
    return tuple(dict.fromkeys((r1, r2, r3)))


@functools.lru_cache(maxsize=None)
def iso_inputs():
    """E2' points (the SSWU outputs of every u above), then (pole, y) for y = 1 and another y"""
    pts = [ref_sswu(u) for u in sswu_us()]
    return tuple(pts) + pole_points()


def pole_points():
    return tuple((r, y) for r in iso_poles() for y in ((1, 0), (P - 2, 5)))


def check_iso_aff(q, out):
    want = O.iso_map(q)
    if out[0] != int(want is None):
        return f"inf = {out[0]}, want {int(want is None)}"
    if want is not None:
        got, err = fps_out(out, XY, at=1)
        return err or _cmp(XY, got, _flat(want))


XYZ = ("X.c0", "X.c1", "Y.c0", "Y.c1", "Z.c0", "Z.c1")


def jac_to_affine(v):
    """affine point of plain Jacobian coordinates [X0, X1, Y0, Y1, Z0, Z1]; None for Z = 0"""
    X, Y, Z = (v[0], v[1]), (v[2], v[3]), (v[4], v[5])
    if O.f2_is_zero(Z):
        return None
    zi = O.f2_inv(Z)
    zi2 = O.f2_sqr(zi)
    return (O.f2_mul(X, zi2), O.f2_mul(Y, O.f2_mul(zi2, zi)))


def check_iso_jac(q, out):
    want = O.iso_map(q)
    got, err = fps_out(out, XYZ)
    if err:
        return err
    aff = jac_to_affine(got)
    if (aff is None) != (want is None):
        return f"Z {'==' if aff is None else '!='} 0, want {'infinity' if want is None else 'a finite point'}"
    if want is not None:
        return _cmp(("X/Z^2 .c0", "X/Z^2 .c1", "Y/Z^3 .c0", "Y/Z^3 .c1"), _flat(aff), _flat(want))


# ---- cofactor clearing -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clear_inputs():
    """(name, E2 point or None): infinity; iso of 32 SSWU points; points already in G2;
    the small-order points of tests/_groupedge.py (order 13, order 23)"""
    _d, rand = sswu_inputs()
    recs = [("infinity", None)]
    recs += [(f"iso(sswu(random u {k}))", O.iso_map(ref_sswu(u))) for k, u in enumerate(rand[:32])]
    rng = random.Random(0xC1EA)
    recs += [(f"[{k:#x}]g2", O.E2.mul(O.G2, k)) for k in (1, 2, O.R - 1, rng.randrange(O.R), rng.randrange(O.R))]
    recs.append(("H('in G2')", O.hash_to_g2(b"in G2".ljust(32, b"."))))
    recs += [(f"order 13, multiple {k}", q) for k, q in zip((1, 2, 12), (ge.q13_multiples()[i] for i in (0, 1, 11)))]
    recs += [(f"order 23, multiple {k}", q) for k, q in zip((1, 2, 22), (ge.q23_multiples()[i] for i in (0, 1, 5)))]
    return tuple(recs)


def pack_point(pt) -> list[int]:
    """inf word, x, y"""
    return [1] + [0] * 48 if pt is None else [0] + pack_fps(_flat(pt))


@functools.lru_cache(maxsize=None)
def ref_clear(pt):
    return None if pt is None else O.clear_cofactor_g2(pt)


def check_point(want, out):
    if out[0] != int(want is None):
        return f"inf = {out[0]}, want {int(want is None)}"
    if want is not None:
        got, err = fps_out(out, XY, at=1)
        return err or _cmp(XY, got, _flat(want))


# ---- k_chain role 0 ----------------------------------------------------------------------------------
def chain_messages() -> list[bytes]:
    rng = random.Random(0xC4A1)
    return [rng.randbytes(32) for _ in range(64)]


@functools.lru_cache(maxsize=None)
def ref_chain_h(q0, q1):
    """H = clear_cofactor(iso(q0) + iso(q1)) (None: H = O, chain_st byte 1)"""
    return ref_clear(O.E2.add(O.iso_map(q0), O.iso_map(q1)))


@functools.lru_cache(maxsize=None)
def chain_directed():
    """(name, q0, q1) with E2' points from the oracle: the branches of the one general
    addition iso(q0) + iso(q1) and the Z == 0 exit of the isogeny"""
    _d, rand = sswu_inputs()
    qa, qb, qc = (ref_sswu(u) for u in rand[:3])
    poles = pole_points()
    recs = [("ordinary", qa, qb), ("q1 == q0 (doubling)", qa, qa), ("q1 == -q0 (H = O)", qb, O.E2_ISO.neg(qb))]
    recs += [(f"q0 at pole ({k}), q1 ordinary", p, qc) for k, p in enumerate(poles)]
    recs += [("q0 ordinary, q1 at pole", qc, poles[0]), ("both at the pole, same y", poles[0], poles[0]),
             ("both at the pole", poles[0], poles[1])]
    return tuple(recs)


def pack_qq(q0, q1) -> list[int]:
    return pack_fps(_flat(q0) + _flat(q1))


def check_chain_h(want, out):
    """out: chain_st byte (1: H = O; HQ is then left as the caller zeroed it), HQ"""
    if out[0] != int(want is None):
        return f"chain_st = {out[0]}, want {int(want is None)}"
    if want is None:
        return None if not any(out[1:49]) else "HQ written although H = O"
    names = tuple("HQ." + c for c in XY)
    got, err = fps_out(out, names, at=1)
    return err or _cmp(names, got, _flat(want))


# ---- Miller loops and final exponentiations through the production launchers ------------------
MILLER, FE = 8, 9
MLF_PAIR = 3  # bls/plan_shape.hpp: two lanes per item (k_mlf2)
PER_LANES = (1, 2, 4, MLF_PAIR)
# product domains of consecutive items: every size 1..5, laid out so that 2 and 4 items per
# lane both meet whole groups of one domain (shared f), groups that straddle two domains
# (every item its own f), and -- 27 items, not a multiple of 4 -- a last lane of three
# items of one domain (the odd tail of the shared loop) resp. of one item
DOMAIN_SIZES = (4, 4, 2, 5, 1, 3, 5, 3)
F12_NAMES = tuple(f"f.c{h}.c{k}.c{j}" for h in (0, 1) for k in (0, 1, 2) for j in (0, 1))
_F12_ORDER = (0, 2, 4, 1, 3, 5)  # Fp12 memory order (c0.c0, c0.c1, c0.c2, c1.c0, ..) in w-basis coefficients


def f12_pack(f) -> list[int]:
    return pack_fps([c for k in _F12_ORDER for c in f[k]])


def f12_unpack(vals):
    """12 plain residues in Fp12 memory order -> the oracle's coefficient list"""
    f = [None] * 6
    for n, k in enumerate(_F12_ORDER):
        f[k] = (vals[2 * n], vals[2 * n + 1])
    return f


@functools.lru_cache(maxsize=None)
def miller_items():
    """(P affine, z, Q affine, domain) per item: P = [k]g1 given with a random Jacobian z or
    z = 1, Q = H(m) or [k]g2"""
    rng = random.Random(0x311E)
    doms = [d for d, n in enumerate(DOMAIN_SIZES) for _ in range(n)]
    items = []
    for i, d in enumerate(doms):
        pa = O.E1.mul(O.G1, rng.randrange(1, 1 << 32))  # (short scalars: the oracle's ladder is slow)
        z = 1 if i % 3 == 1 else rng.randrange(1, P)
        q = O.hash_to_g2(rng.randbytes(32)) if i % 2 == 0 else O.E2.mul(O.G2, rng.randrange(1, 1 << 32))
        items.append((pa, z, q, 0x40 + d))
    assert len(items) == 27
    return tuple(items)


def pack_miller(item, per_lane: int) -> list[int]:
    (x, y), z, q, dom = item
    return pack_fps([x * z * z % P, y * z * z * z % P, z]) + pack_fps(_flat(q)) + [dom, per_lane]


def miller_shared(per_lane: int, doms) -> dict:
    """item -> the items whose product its f holds ([] for an item whose f must be exactly 1),
    by kernels/k_mlq.hip mlf_lane: the items of a lane share one f when there are at least
    two and all are of one domain; two lanes per item (MLF_PAIR) never share"""
    n = len(doms)
    holds = {}
    pl = 1 if per_lane == MLF_PAIR else per_lane
    for k0 in range(0, n, pl):
        grp = list(range(k0, min(k0 + pl, n)))
        if len(grp) > 1 and len({doms[i] for i in grp}) == 1:
            holds[k0] = grp
            for i in grp[1:]:
                holds[i] = []
        else:
            for i in grp:
                holds[i] = [i]
    return holds


@functools.lru_cache(maxsize=None)
def ref_miller(i: int):
    pa, _z, q, _d = miller_items()[i]
    return O.miller_loop(pa, q)


def f12_prod(fs):
    acc = O.F12_ONE
    for f in fs:
        acc = O.f12_mul(acc, f)
    return acc


@functools.lru_cache(maxsize=None)
def ref_domain_fe(d: int):
    """FE(prod of the oracle's Miller values over domain d), the exponent 3 (p^12 - 1)/r"""
    items = miller_items()
    return O.final_exponentiation(f12_prod([ref_miller(i) for i in range(len(items)) if items[i][3] == 0x40 + d]), 3)


def check_miller(per_lane: int, out_rows, what: str):
    """out_rows: one list of 144 words per item of miller_items().  Every f canonical; an
    item that shared another's f exactly 1; per domain FE(prod f) equal to the oracle's."""
    items = miller_items()
    doms = [it[3] for it in items]
    holds = miller_shared(per_lane, doms)
    fs = []
    for i, row in enumerate(out_rows):
        vals, err = fps_out(row, F12_NAMES)
        if err:
            return f"{what}, item {i}: {err}"
        f = f12_unpack(vals)
        if not holds[i] and f != O.F12_ONE:
            return f"{what}, item {i}: shared the f of item {max(k for k in holds if holds[k] and i in holds[k])} and must hold exactly 1, holds {hx(f)}"
        fs.append(f)
    for d in range(len(DOMAIN_SIZES)):
        got = O.final_exponentiation(f12_prod([fs[i] for i in range(len(items)) if doms[i] == 0x40 + d]), 3)
        if got != ref_domain_fe(d):
            members = [i for i in range(len(items)) if doms[i] == 0x40 + d]
            return f"{what}, domain {d} (items {members}): FE(prod f) differs from FE(prod of the oracle's Miller loops)"


@functools.lru_cache(maxsize=None)
def bilinear_items():
    """f(aP, Q) and f(P, aQ), each its own domain"""
    rng = random.Random(0xB111)
    a = rng.randrange(2, O.R)
    pa, q = O.E1.mul(O.G1, rng.randrange(1, O.R)), O.hash_to_g2(b"bilinear".ljust(32, b"-"))
    return ((O.E1.mul(pa, a), rng.randrange(1, P), q, 1), (pa, 1, O.E2.mul(q, a), 2))


@functools.lru_cache(maxsize=None)
def fe_tasks():
    """(name, F): 16 values whose FE is 1 by construction, is not by construction, or is
    whatever the oracle says -- and three r-th powers.  A verdict bit sees a wrong exponent in
    the hard part only on an F whose FE is 1 while its easy part t is not: the cancelling
    pairs' products lie in Fp6, so their t is 1 and every power of it too, and a random F
    gives "not 1" under almost any exponent.  G^r has FE = FE(G)^r = 1 with t of a large
    order dividing (p^4 - p^2 + 1) / r, which a wrong exponent does not kill."""
    rng = random.Random(0xFE16)

    def fp6_unit():
        return [(rng.randrange(P), rng.randrange(P)) if k % 2 == 0 else O.F2_ZERO for k in range(6)]

    tasks = [("one", list(O.F12_ONE))]
    pairs = []
    for k in range(3):
        pa = O.E1.mul(O.G1, rng.randrange(1, O.R))
        q = O.E2.mul(O.G2, rng.randrange(1, O.R)) if k else O.hash_to_g2(b"fe".ljust(32, b"+"))
        pairs.append((O.miller_loop(pa, q), O.miller_loop(O.E1.neg(pa), q), O.miller_loop(O.E1.dbl(pa), q)))
    tasks += [(f"cancelling pair {k}", O.f12_mul(m, mn)) for k, (m, mn, _o) in enumerate(pairs)]
    tasks += [(f"cancelling pair {k} times an element of Fp6", O.f12_mul(O.f12_mul(m, mn), fp6_unit()))
              for k, (m, mn, _o) in enumerate(pairs)]
    tasks += [(f"pair {k} with one factor replaced, times an element of Fp6", O.f12_mul(O.f12_mul(m, o), fp6_unit()))
              for k, (m, _mn, o) in enumerate(pairs)]
    tasks += [(f"random {k}", [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]) for k in range(6)]
    assert len(tasks) == 16
    tasks += [(f"r-th power {k}", O.f12_pow([(rng.randrange(P), rng.randrange(P)) for _ in range(6)], O.R))
              for k in range(3)]
    return tuple((nm, tuple(f)) for nm, f in tasks)


@functools.lru_cache(maxsize=None)
def ref_fe_is_one(k: int) -> bool:
    return O.f12_is_one(O.final_exponentiation(list(fe_tasks()[k][1]), 3))


# ---- the sets ------------------------------------------------------------------------------------------
@dataclass
class VectorSet:
    name: str
    op: int
    flavours: tuple  # 0: the 32-bit column product, D28: the 28-bit-digit one
    tu: str | None   # fixed translation unit (the k_chain.hip ops), else by flavour
    records: Callable  # () -> list of records
    pack: Callable     # record -> list of uint32 words
    check: Callable    # (record, output words as Python ints) -> None or a description
    label: Callable    # record -> str for failure messages

    def where(self, flavour: int) -> str:
        return self.tu or TU[flavour]


def _sets():
    S = VectorSet
    return [
        S("from_be64", FROM_BE64, (0, D28), None, from_be64_values, pack_be64, check_from_be64, hx),
        S("h2f", H2F, (0, D28), None, h2f_messages, pack_msg, check_h2f, lambda m: m.hex()),
        S("sswu", SSWU, (0,), None, sswu_us, lambda u: pack_f2s(u), check_sswu, hx),
        S("sswu_fast", SSWU_FAST, (D28,), None, sswu_us, lambda u: pack_f2s(u), check_sswu_fast, hx),
        S("iso_aff", ISO_AFF, (0,), None, lambda: list(iso_inputs()), lambda q: pack_f2s(*q), check_iso_aff, hx),
        S("iso_jac", ISO_JAC, (D28,), TU_CHAIN, lambda: list(iso_inputs()), lambda q: pack_f2s(*q), check_iso_jac, hx),
        S("clear_cofactor", CLEAR_COFACTOR, (0,), None, lambda: list(clear_inputs()), lambda r: pack_point(r[1]),
          lambda r, out: check_point(ref_clear(r[1]), out), lambda r: f"{r[0]} {hx(r[1])}"),
        S("chain_h", CHAIN_H, (D28,), TU_CHAIN, lambda: list(chain_directed()), lambda r: pack_qq(r[1], r[2]),
          lambda r, out: check_chain_h(ref_chain_h(r[1], r[2]), out), lambda r: f"{r[0]}: q0 = {hx(r[1])}, q1 = {hx(r[2])}"),
    ]


SETS = {s.name: s for s in _sets()}
SET_NAMES = tuple(SETS)
FLAVOUR_ID = {0: "cols", D28: "d28"}
CASES = [(s.name, fl) for s in SETS.values() for fl in s.flavours]
CASE_IDS = [f"{nm}-{'chain' if SETS[nm].tu else FLAVOUR_ID[fl]}" for nm, fl in CASES]


def failure(s: VectorSet, flavour: int, i: int, rec, err: str) -> str:
    return f"{s.name} in {s.where(flavour)}, record {i} [{s.label(rec)}]: {err}"
