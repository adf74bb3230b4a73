"""Point encodings at the field and flag-byte edges: named byte strings for the three
decoders of csrc/bls/curve.hpp (g2_decompress96, g1_decompress48, g1_deserialize96),
built on the CPU, with every expected value taken from oracle/bls_oracle.py:

* decode codes and points from g2_decompress, g1_decompress, g1_deserialize;
* validate codes from signature_from_bytes (validate=True) and key_validate;
* subgroup membership (inside those two) from g2_in_subgroup, g1_in_subgroup.

Nothing here comes from the library under test.  tests/test_wirevec_cpu.py checks the set
itself and runs it through the CPU build of the same headers; tests/test_gpu_wire_edges.py
sends it through every GPU entry point that takes bytes from outside.

The three lists are longer than 64 and no multiple of 64, so one launch over a list has a
full and a partial wavefront.  Names are unique within a list; a failure is reported by
the vector's name."""
from __future__ import annotations

import functools
import hashlib
from dataclasses import dataclass

from oracle import bls_oracle as O

P = O.P
HALF = (P - 1) // 2
T381 = 1 << 381
# index i of the message sha256(b"%d" % i) whose signature by interop key 0 has
# x.c0 + p < 2^381 (S0) / x.c1 + p < 2^381 (S1), and the interop key whose x + p < 2^381
# (K); about 19 % qualify.  Found by the searches below, which assert these values.
S0_INDEX, S1_INDEX, K_INDEX, K2_INDEX = 4, 0, 2, 3
SEARCH = 64


@dataclass(frozen=True)
class Vec:
    name: str
    data: bytes
    code: int  # the oracle's decode code
    point: object  # the oracle's point (None: infinity, or no point when code != 0)
    vcode: int  # the oracle's validate code (signature_from_bytes validate=True / key_validate)


def msg_of(i: int) -> bytes:
    return hashlib.sha256(b"%d" % i).digest()


def _b48(v: int) -> bytes:
    return v.to_bytes(48, "big")


def g2_bytes(c0: int, c1: int, flags: int) -> bytes:
    """x.c1 (below 2^381, under the three flag bits `flags` of byte 0) || x.c0 (any 384-bit value)"""
    assert 0 <= c1 < T381 and 0 <= c0 < 1 << 384 and flags & ~0xE0 == 0
    b = bytearray(_b48(c1) + _b48(c0))
    b[0] |= flags
    return bytes(b)


def g1_bytes(x: int, flags: int) -> bytes:
    assert 0 <= x < T381 and flags & ~0xE0 == 0
    b = bytearray(_b48(x))
    b[0] |= flags
    return bytes(b)


def _sig_vcode(b: bytes) -> int:
    try:
        O.signature_from_bytes(b)
    except O.BlsError as e:
        return e.code
    return O.E_OK


def _g2(name: str, b: bytes) -> Vec:
    code, pt = O.g2_decompress(b)
    return Vec(name, b, code, pt, _sig_vcode(b))


def _g1c(name: str, b: bytes) -> Vec:
    code, pt = O.g1_decompress(b)
    return Vec(name, b, code, pt, O.key_validate(b))


def _g1u(name: str, b: bytes) -> Vec:
    code, pt = O.g1_deserialize(b)
    return Vec(name, b, code, pt, O.key_validate(b))


def limb_walk(base_name: str):
    """(name, value) of p + 2^(32k) and p - 2^(32k), k = 0..11: a canonical check that skips
    a limb, or loses a borrow in one, answers one of these wrongly"""
    for k in range(12):
        yield "%s=p+2^%d" % (base_name, 32 * k), P + (1 << (32 * k))
        yield "%s=p-2^%d" % (base_name, 32 * k), P - (1 << (32 * k))


# ---- sources ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def alias_signature(sk: int, coord: int, first: int = 0):
    """(i, compressed signature of msg_of(i) by sk) for the first i >= first (at most SEARCH
    tried) whose x.c<coord> + p stays below 2^381: that signature has a non-canonical alias
    with the same flag bits"""
    for i in range(first, first + SEARCH):
        pt = O.sign(sk, msg_of(i))
        if pt[0][coord] + P < T381:
            return i, O.g2_compress(pt)
    raise AssertionError("no signature with x.c%d + p < 2^381 in %d tries" % (coord, SEARCH))


def alias_of(sig: bytes, coord: int) -> bytes:
    """sig with x.c<coord> replaced by x.c<coord> + p (flag bits unchanged)"""
    c1 = int.from_bytes(bytes([sig[0] & 0x1F]) + sig[1:48], "big")
    c0 = int.from_bytes(sig[48:], "big")
    return g2_bytes(c0 + P if coord == 0 else c0, c1 + P if coord == 1 else c1, sig[0] & 0xE0)


@functools.lru_cache(maxsize=None)
def alias_key():
    """(interop index, secret key, point) of the first interop key with x + p < 2^381"""
    for i in range(SEARCH):
        sk = O.interop_secret_key(i)
        pt = O.sk_to_pk(sk)
        if pt[0] + P < T381:
            return i, sk, pt
    raise AssertionError("no interop key with x + p < 2^381")


@functools.lru_cache(maxsize=None)
def real_y_points():
    """(x with y.c1 == 0, x with y.c0 == 0) on E2.  For x = a + b u, x^3 + 4 (1 + u) is real
    exactly when 3 a^2 b - b^3 = -4, i.e. a^2 = (b^3 - 4) / (3 b); its square root then lies
    in Fp (y.c1 == 0) or in u Fp (y.c0 == 0)."""
    c1_zero = c0_zero = None
    b = 1
    while c1_zero is None or c0_zero is None:
        a = O.fp_sqrt((b ** 3 - 4) * pow(3 * b, -1, P))
        for root in ([] if a is None else [a, (-a) % P]):
            x = (root, b)
            assert O.f2_add(O.f2_mul(O.f2_sqr(x), x), O.B2)[1] == 0
            code, pt = O.g2_decompress(g2_bytes(x[0], x[1], 0x80))
            assert code == O.E_OK  # every element of Fp is a square in Fp2
            if pt[1][1] == 0 and c1_zero is None:
                c1_zero = x
            if pt[1][0] == 0 and c0_zero is None:
                c0_zero = x
        b += 1
        assert b < 64
    return c1_zero, c0_zero


def _off_curve_t(c1: int) -> int:
    """the smallest t with (t, c1) no x coordinate of E2"""
    for t in range(64):
        if O.g2_decompress(g2_bytes(t, c1, 0x80))[0] == O.E_POINT_NOT_ON_CURVE:
            return t
    raise AssertionError("no off-curve x")


INF_STRAY_G2 = (1, 47, 48, 95)
INF_STRAY_G1 = (1, 24, 47)


def _infinity_strays(n: int, first: int, offsets):
    """(name, bytes): the infinity encoding of n bytes with one stray 0x01, and with a stray
    low bit in the flag byte"""
    for off in offsets:
        b = bytearray(n)
        b[0], b[off] = first, b[off] | 1
        yield "inf_stray@%d" % off, bytes(b)
    yield "inf_flag_byte_%02x" % (first | 1), bytes([first | 1]) + bytes(n - 1)


# ---- the lists -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g2_vectors() -> tuple:
    sk0 = O.interop_secret_key(0)
    i0, s0 = alias_signature(sk0, 0)
    i1, s1 = alias_signature(sk0, 1)
    assert (i0, i1) == (S0_INDEX, S1_INDEX)
    flags = s0[0] & 0xE0
    c1 = int.from_bytes(bytes([s0[0] & 0x1F]) + s0[1:48], "big")
    c0 = int.from_bytes(s0[48:], "big")
    out = [_g2("canon", s0), _g2("sort_flip", bytes([s0[0] ^ 0x20]) + s0[1:]),
           _g2("alias_c0", alias_of(s0, 0)), _g2("alias_c1", alias_of(s1, 1))]
    for bit in (7, 5):  # the lower half carries no flags: plain values >= p
        b = bytearray(s0)
        b[48] |= 1 << bit
        out.append(_g2("c0_high_bits/bit%d" % bit, bytes(b)))
    edges = (("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2^381-1", T381 - 1))
    out += [_g2("c0=" + nm, g2_bytes(v, c1, flags)) for nm, v in edges + (("2^384-1", (1 << 384) - 1),)]
    out += [_g2("c1=" + nm, g2_bytes(c0, v, flags)) for nm, v in edges]
    out += [_g2(nm, g2_bytes(v, c1, flags)) for nm, v in limb_walk("c0")]
    out += [_g2(nm, g2_bytes(c0, v, flags)) for nm, v in limb_walk("c1")]
    # blst checks the encoding before the curve equation
    out.append(_g2("precedence", g2_bytes(P + _off_curve_t(c1), c1, flags)))
    for f in range(8):
        out.append(_g2("flags_%02x/zero_body" % (f << 5), g2_bytes(0, 0, f << 5)))
        out.append(_g2("flags_%02x/s0_body" % (f << 5), g2_bytes(c0, c1, f << 5)))
    out += [_g2(nm, b) for nm, b in _infinity_strays(96, 0xC0, INF_STRAY_G2)]
    xr, xi = real_y_points()
    for nm, x in (("y.c1=0", xr), ("y.c0=0", xi)):
        out += [_g2("%s/sort%d" % (nm, s), g2_bytes(x[0], x[1], 0x80 | (s << 5))) for s in (0, 1)]
    return _checked(out)


@functools.lru_cache(maxsize=None)
def g1_compressed_vectors() -> tuple:
    ki, _, (x, y) = alias_key()
    assert ki == K_INDEX
    k = O.g1_compress((x, y))
    flags = k[0] & 0xE0
    out = [_g1c("canon", k), _g1c("sort_flip", bytes([k[0] ^ 0x20]) + k[1:]), _g1c("alias", g1_bytes(x + P, flags))]
    out += [_g1c("x=" + nm, g1_bytes(v, flags)) for nm, v in
            (("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2^381-1", T381 - 1))]
    out += [_g1c(nm, g1_bytes(v, flags)) for nm, v in limb_walk("x")]
    t = next(t for t in range(64) if O.g1_decompress(g1_bytes(t, 0x80))[0] == O.E_POINT_NOT_ON_CURVE)
    out.append(_g1c("precedence", g1_bytes(P + t, flags)))
    for f in range(8):
        out.append(_g1c("flags_%02x/zero_body" % (f << 5), g1_bytes(0, f << 5)))
        out.append(_g1c("flags_%02x/k_body" % (f << 5), g1_bytes(x, f << 5)))
    out += [_g1c(nm, b) for nm, b in _infinity_strays(48, 0xC0, INF_STRAY_G1)]
    # ordinary keys, so that valid lanes sit between the rejected ones
    out += [_g1c("interop_%d" % i, O.g1_compress(O.sk_to_pk(O.interop_secret_key(i)))) for i in range(16) if i != ki]
    return _checked(out)


@functools.lru_cache(maxsize=None)
def g1_uncompressed_vectors() -> tuple:
    ki, _, (x, y) = alias_key()
    x2, y2 = O.sk_to_pk(O.interop_secret_key(K2_INDEX))
    assert K2_INDEX != ki

    def u(xv, yv, top=0):
        b = bytearray(_b48(xv) + _b48(yv))
        b[0] |= top
        return bytes(b)

    out = [_g1u("canon", u(x, y)), _g1u("neg", u(x, P - y)), _g1u("alias_x", u(x + P, y)),
           _g1u("alias_y", u(x, (y + P) % (1 << 384))), _g1u("x=p", u(P, y)), _g1u("y=p", u(x, P)),
           _g1u("y=p-1", u(x, P - 1))]
    out += [_g1u(nm, u(x, v)) for nm, v in limb_walk("y")]
    out += [_g1u(nm, u(v, y)) for nm, v in limb_walk("x")]
    out.append(_g1u("off_curve", u(x, y2)))
    out.append(_g1u("precedence", u(x + P, y2)))
    for top in (0x80, 0x40, 0x20):
        out.append(_g1u("top_%02x/k_body" % top, u(x, y, top)))
        out.append(_g1u("top_%02x/zero_body" % top, u(0, 0, top)))
    out += [_g1u(nm, b) for nm, b in _infinity_strays(96, 0x40, INF_STRAY_G2)]
    return _checked(out)


def _checked(vecs) -> tuple:
    names = [v.name for v in vecs]
    assert len(set(names)) == len(names), "duplicate vector names"
    assert len(vecs) > 64 and len(vecs) % 64 != 0, len(vecs)
    return tuple(vecs)


def by_name(vecs) -> dict:
    return {v.name: v for v in vecs}
