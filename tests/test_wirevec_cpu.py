"""The wire-edge vectors (tests/_wirevec.py) checked on the CPU: first the set itself, so
it cannot degenerate silently (an alias that is no alias, a source that is no valid
signature, a decoder code that no vector produces), then the same vectors through the CPU
build of the same headers (tests/native/hostsim.cpp): codes equal to the oracle's, points
bit-exact, and compress(decompress(b)) == b for everything that decodes."""
from __future__ import annotations

import ctypes

import pytest

from tests import _wirevec as W
from tests._codec import P, g1b, g2b

E_OK, E_BAD, E_CURVE, E_GROUP = 0, 1, 2, 3


def _x_of_g2(b: bytes):
    return int.from_bytes(b[48:], "big"), int.from_bytes(bytes([b[0] & 0x1F]) + b[1:48], "big")


# ---- the set itself ----------------------------------------------------------------------------
def test_list_lengths():
    for vecs in (W.g2_vectors(), W.g1_compressed_vectors(), W.g1_uncompressed_vectors()):
        assert len(vecs) > 64 and len(vecs) % 64 != 0
    assert all(len(v.data) == 96 for v in W.g2_vectors() + W.g1_uncompressed_vectors())
    assert all(len(v.data) == 48 for v in W.g1_compressed_vectors())


def test_every_decoder_code_occurs():
    for vecs in (W.g2_vectors(), W.g1_compressed_vectors(), W.g1_uncompressed_vectors()):
        assert {v.code for v in vecs} == {E_OK, E_BAD, E_CURVE}
        assert any(v.code == E_OK and v.point is None for v in vecs)  # infinity
    for vecs in (W.g2_vectors(), W.g1_compressed_vectors()):  # on the curve, outside the group
        assert any(v.code == E_OK and v.vcode == E_GROUP for v in vecs)


def test_g2_aliases(oracle, golden):
    g2 = W.by_name(W.g2_vectors())
    canon = g2["canon"]
    assert canon.code == E_OK and canon.vcode == E_OK  # a valid signature, in G2
    assert canon.point == oracle.sign(oracle.interop_secret_key(0), W.msg_of(W.S0_INDEX))
    assert g2["sort_flip"].point == (canon.point[0], oracle.f2_neg(canon.point[1])) and g2["sort_flip"].vcode == E_OK
    a0, a1 = g2["alias_c0"], g2["alias_c1"]
    c0, c1 = _x_of_g2(a0.data)
    assert c0 >= P and (c0 % P, c1) == canon.point[0] and a0.data[0] & 0xE0 == canon.data[0] & 0xE0
    _, s1 = W.alias_signature(oracle.interop_secret_key(0), 1)
    assert oracle.signature_from_bytes(s1) == oracle.sign(oracle.interop_secret_key(0), W.msg_of(W.S1_INDEX))
    c0, c1 = _x_of_g2(a1.data)
    assert c1 >= P and (c0, c1 % P) == _x_of_g2(s1) and a1.data[0] & 0xE0 == s1[0] & 0xE0
    for v in (a0, a1, g2["c0_high_bits/bit7"], g2["c0_high_bits/bit5"], g2["precedence"]):
        assert v.code == E_BAD and v.vcode == E_BAD, v.name
    # the precedence vector reduces to an x that is on no curve point
    c0, c1 = _x_of_g2(g2["precedence"].data)
    assert c0 >= P and oracle.g2_decompress(W.g2_bytes(c0 - P, c1, 0x80))[0] == E_CURVE
    for nm, v in g2.items():
        if "=p+2^" in nm:
            assert v.code == E_BAD, nm


def test_g2_real_y_points(oracle):
    g2 = W.by_name(W.g2_vectors())
    for nm, zero in (("y.c1=0", 1), ("y.c0=0", 0)):
        s0, s1 = g2[nm + "/sort0"], g2[nm + "/sort1"]
        assert s0.code == s1.code == E_OK
        assert s0.point[1][zero] == 0 and s0.point[1][1 - zero] != 0
        assert s1.point == (s0.point[0], oracle.f2_neg(s0.point[1]))
        assert oracle.E2.on_curve(s0.point) and not oracle.lex_largest_f2(s0.point[1])
        assert s0.vcode == (E_OK if oracle.g2_in_subgroup(s0.point) else E_GROUP)


def test_g1_aliases(oracle, golden):
    ki, sk, pt = W.alias_key()
    assert oracle.g1_compress(pt).hex() == golden["kat2_interop_pubkeys"][ki]
    c = W.by_name(W.g1_compressed_vectors())
    assert c["canon"].point == pt and c["canon"].vcode == E_OK
    assert c["sort_flip"].point == (pt[0], P - pt[1]) and c["sort_flip"].vcode == E_OK
    x = int.from_bytes(bytes([c["alias"].data[0] & 0x1F]) + c["alias"].data[1:], "big")
    assert x == pt[0] + P and c["alias"].data[0] & 0xE0 == c["canon"].data[0] & 0xE0
    assert c["alias"].code == c["alias"].vcode == c["precedence"].code == E_BAD
    u = W.by_name(W.g1_uncompressed_vectors())
    assert u["canon"].point == pt and u["neg"].point == (pt[0], P - pt[1]) and u["canon"].vcode == u["neg"].vcode == E_OK
    for nm, k in (("alias_x", 0), ("alias_y", 1)):
        xy = (int.from_bytes(u[nm].data[:48], "big"), int.from_bytes(u[nm].data[48:], "big"))
        assert xy[k] == pt[k] + P and xy[1 - k] == pt[1 - k] and u[nm].code == u[nm].vcode == E_BAD
    assert u["off_curve"].code == E_CURVE and u["precedence"].code == E_BAD
    assert u["top_40/zero_body"].code == E_OK and u["top_40/zero_body"].point is None
    for vecs in (c, u):
        for nm, v in vecs.items():
            if "=p+2^" in nm:
                assert v.code == E_BAD, nm


# ---- the CPU build of the device's decoders ----------------------------------------------------
def _decode(fn, data: bytes, out_len: int):
    out = ctypes.create_string_buffer(out_len)
    return fn(data, out), out.raw


def test_g2_decompress_hostsim(hostsim):
    for v in W.g2_vectors():
        code, raw = _decode(hostsim.hs_g2_decompress, v.data, 192)
        assert code == v.code, "%s: code %d, oracle %d" % (v.name, code, v.code)
        if code != E_OK:
            continue
        assert raw == g2b(v.point), "%s: point %s" % (v.name, raw.hex())
        back = ctypes.create_string_buffer(96)
        hostsim.hs_g2_compress(raw, back)
        assert back.raw == v.data, "%s: g2_compress96 gives %s" % (v.name, back.raw.hex())


def test_g1_decompress_hostsim(hostsim, oracle):
    for v in W.g1_compressed_vectors():
        code, raw = _decode(hostsim.hs_g1_decompress, v.data, 96)
        assert code == v.code, "%s: code %d, oracle %d" % (v.name, code, v.code)
        if code != E_OK:
            continue
        assert raw == g1b(v.point), "%s: point %s" % (v.name, raw.hex())
        back = ctypes.create_string_buffer(48)
        hostsim.hs_g1_compress(raw, back)
        assert back.raw == v.data, "%s: g1_compress48 gives %s" % (v.name, back.raw.hex())


def test_g1_deserialize_hostsim(hostsim, oracle):
    for v in W.g1_uncompressed_vectors():
        code, raw = _decode(hostsim.hs_g1_deserialize, v.data, 96)
        assert code == v.code, "%s: code %d, oracle %d" % (v.name, code, v.code)
        if code != E_OK:
            continue
        assert raw == g1b(v.point) == v.data, "%s: point %s" % (v.name, raw.hex())
        back = ctypes.create_string_buffer(48)
        hostsim.hs_g1_compress(raw, back)
        assert back.raw == oracle.g1_compress(v.point), "%s: g1_compress48 gives %s" % (v.name, back.raw.hex())
