"""The inputs of tests/test_gpu_group_edges.py are what tests/_groupedge.py claims, proved
against the oracle on the CPU: the orders of the low-order points and that they lie
outside G1 / G2, which additions of the [|x|] chain they make exceptional, the negation
encodings, the infinity serializations, the index-list layouts and the reference's verdict
for an aggregate key at infinity."""
from __future__ import annotations

import hashlib

import pytest

from tests import _groupedge as ge


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


# ---------------------------------------------------------------------------
# low-order points
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [13, 23])
def test_low_order_e2_point(oracle, ell):
    O = oracle
    x1, pt, T = ge.low_order_e2(ell)
    assert O.E2.on_curve(pt) and O.E2.on_curve(T)
    assert O.E2.mul(pt, ge.N2) is None, "the cofactor constant H2 is wrong: [H2 r]pt != O"
    assert ge.N2 % (ell * ell) == 0 and ge.N2 % ell ** 3 != 0
    assert T is not None and O.E2.mul(T, ell) is None          # order exactly ell (prime)
    assert not O.g2_in_subgroup(T)
    with pytest.raises(O.BlsError) as e:
        O.signature_from_bytes(O.g2_compress(T), validate=True)
    assert e.value.code == O.E_POINT_NOT_IN_GROUP == 3
    assert O.signature_from_bytes(O.g2_compress(T), validate=False) == T
    if ell == 13:
        assert x1 == 2
        c = O.g2_compress(T).hex()
        assert c.startswith("ae074268") and c.endswith("6b139784")


def test_low_order_e2_multiples(oracle):
    O = oracle
    m13, m23 = ge.q13_multiples(), ge.q23_multiples()
    assert len(m13) == 12 and len(set(m13)) == 12 and None not in m13
    for k, q in enumerate(m13, start=1):
        assert O.E2.add(q, m13[12 - k]) is None, k          # [k]T + [13 - k]T = O: both signs present
        assert O.E2.mul(q, 13) is None and not O.g2_in_subgroup(q)
    assert len(set(m23)) == len(m23) >= 3 and None not in m23
    assert O.E2.add(m23[0], m23[-1]) is None                # T and [22]T = -T
    for q in m23:
        assert O.E2.mul(q, 23) is None and not O.g2_in_subgroup(q)
    s13, s23 = ge.low_order_sigs()
    for raw, q in zip(s13 + s23, m13 + m23):
        assert O.g2_decompress(raw) == (O.E_OK, q)
        with pytest.raises(O.BlsError) as e:
            O.signature_from_bytes(raw, validate=True)
        assert e.value.code == 3


def test_low_order_e1_points(oracle):
    O = oracle
    for q in ge.ORDER3_E1:
        assert O.E1.on_curve(q) and O.E1.mul(q, 3) is None and O.E1.dbl(q) == O.E1.neg(q)
        assert not O.g1_in_subgroup(q)
    assert O.E1.add(*ge.ORDER3_E1) is None
    x, pt, T = ge.low_order_e1(11)
    assert O.E1.on_curve(pt) and O.E1.mul(pt, ge.N1) is None, "the cofactor constant H1 is wrong"
    assert ge.N1 % 121 == 0 and ge.N1 % 1331 != 0
    assert T is not None and O.E1.mul(T, 11) is None and not O.g1_in_subgroup(T)
    names = [n for n, _ in ge.low_order_keys()]
    assert len(names) == len(set(names)) == 6
    for name, q in ge.low_order_keys():
        assert q is not None and O.E1.on_curve(q) and not O.g1_in_subgroup(q), name
        assert O.key_validate(O.g1_compress(q)) == O.E_POINT_NOT_IN_GROUP, name
        assert O.key_validate(O.g1_serialize(q)) == O.E_POINT_NOT_IN_GROUP, name


# ---------------------------------------------------------------------------
# the [|x|] chain's exceptional additions
# ---------------------------------------------------------------------------
def test_prefix_walk_is_the_chain(oracle):
    """prefix_walk's bookkeeping is the double-and-add itself: replayed on the order-13
    point with the oracle's complete addition, the accumulator is infinity, P or -P exactly
    where the walk says, and the chain ends at [|x| mod 13]T."""
    O = oracle
    T = ge.low_order_e2(13)[2]
    events = {}
    for i, kind in ge.prefix_walk(13):
        events.setdefault(i, []).append(kind)
    bits = bin(O.X_ABS)[3:]
    acc = T
    for n, bit in enumerate(bits):
        i = len(bits) - 1 - n
        kinds = events.get(i, [])
        assert (acc is None) == ("dbl_inf" in kinds), i
        acc = O.E2.dbl(acc)
        if bit == "1":
            want = "add_inf" if acc is None else "add_dbl" if acc == T else "add_neg" if acc == O.E2.neg(T) else None
            assert [k for k in kinds if k != "dbl_inf"] == ([want] if want else []), i
            acc = O.E2.add(acc, T)
    assert acc == O.E2.mul(T, O.X_ABS % 13)


def test_prefix_collisions_13_and_23():
    """Order 13 collides with the chain (an addition meets -P and gives infinity, the next
    three doublings double infinity, the next addition adds to infinity); order 23 and the
    other small prime factors of the G2 cofactor do not: the order-23 point is the control
    that stays on the ordinary branches.  A change to the chain (another scalar, another
    bit order) that moves these collisions fails here first."""
    w = ge.prefix_walk(13)
    assert w == [(60, "add_neg"), (59, "dbl_inf"), (58, "dbl_inf"), (57, "dbl_inf"), (57, "add_inf")]
    for ell in (23, 2713, 11953, 262069):
        assert ge.prefix_walk(ell) == [], ell


def test_prefix_collisions_3_and_11():
    w3, w11 = ge.prefix_walk(3), ge.prefix_walk(11)
    assert len([k for _, k in w3 if k.startswith("add_")]) >= 2           # several
    assert {"add_neg", "add_inf", "add_dbl", "dbl_inf"} == {k for _, k in w3}
    assert w11 == [(60, "add_dbl")]                                        # one, k = 1 (mod 11)


# ---------------------------------------------------------------------------
# negation and infinity encodings
# ---------------------------------------------------------------------------
def test_negation_encodings(oracle, golden):
    O = oracle
    for h in golden["kat2_interop_pubkeys"][:ge.N_BASE]:
        k = bytes.fromhex(h)
        code, pt = O.g1_decompress(k)
        assert code == 0 and pt[1] != 0
        assert ge.neg_compressed(k) == O.g1_compress(O.E1.neg(pt))
    sigs = [bytes.fromhex(s["sig"]) for s in golden["signatures"]] + list(ge.low_order_sigs()[0])
    for s in sigs:
        pt = O.signature_from_bytes(s, validate=False)
        assert pt[1] != (0, 0)
        assert ge.neg_compressed(s) == O.g2_compress(O.E2.neg(pt))
    for _, q in ge.low_order_keys():
        assert ge.neg_compressed(O.g1_compress(q)) == O.g1_compress(O.E1.neg(q))


def test_infinity_serializations(oracle, golden):
    O = oracle
    k = bytes.fromhex(golden["kat2_interop_pubkeys"][3])
    p = O.g1_decompress(k)[1]
    n = O.g1_decompress(ge.neg_compressed(k))[1]
    agg = O.aggregate_pubkeys([p, n])
    assert agg is None
    assert O.g1_serialize(agg) == ge.INF_PK96 == bytes([0x40]) + bytes(95)
    s = O.signature_from_bytes(bytes.fromhex(golden["signatures"][0]["sig"]))
    ns = O.signature_from_bytes(ge.neg_compressed(bytes.fromhex(golden["signatures"][0]["sig"])))
    assert O.g2_compress(O.E2.add(s, ns)) == ge.INF_SIG96 == bytes([0xC0]) + bytes(95)
    assert O.g1_decompress(ge.INF_PK48) == (O.E_OK, None)      # the table's infinity entry decodes
    assert O.key_validate(ge.INF_PK48) == O.E_PK_IS_INFINITY


# ---------------------------------------------------------------------------
# the table, the lists and their scalars
# ---------------------------------------------------------------------------
def test_table_and_scalars(oracle, golden):
    O = oracle
    keys = ge.table_keys(golden)
    assert len(keys) == ge.INF_INDEX + 1 and keys[ge.INF_INDEX] == ge.INF_PK48
    for i in (0, 7, 31, 32, 39, 40):
        assert O.g1_decompress(keys[i])[1] == O.sk_to_pk(ge.table_sk(i)), i
    lst = [0, 0, 33, 5, ge.INF_INDEX, 32]
    assert ge.expected_aggregate(keys, lst) == O.g1_serialize(O.sk_to_pk(ge.list_sk(lst)))


def test_pk_layouts_do_what_their_names_say(oracle, golden):
    """The lane and tree bookkeeping of k_pk_agg replayed on the CPU with scalars in place
    of points (lane l sums positions l, l + 64, ...; level s adds lane l + s into lane
    l < s): each named layout makes equal or opposite partial sums meet where its name
    says, and the expected sums are infinity where the test wants 0x40 00...."""
    O = oracle
    keys = ge.table_keys(golden)
    lay = dict(ge.pk_layouts())
    assert len(lay) == len(ge.pk_layouts())

    def replay(lst):
        """[(where, kind)] with kind 'dbl' (equal non-zero operands) or 'cancel' (opposite)"""
        assert len(lst) >= ge.AGG_MIN
        ev, part = [], [0] * ge.LANES
        seen = [False] * ge.LANES
        for pos, idx in enumerate(lst):
            l, k = pos % ge.LANES, ge.table_sk(idx)
            if seen[l] and k and part[l]:
                if part[l] == k:
                    ev.append(("lane", "dbl"))
                elif (part[l] + k) % O.R == 0:
                    ev.append(("lane", "cancel"))
            part[l] = (part[l] + k) % O.R
            seen[l] = True
        s = ge.LANES // 2
        while s >= 1:
            for l in range(s):
                a, b = part[l], part[l + s]
                if a and b:
                    if a == b:
                        ev.append((s, "dbl"))
                    elif (a + b) % O.R == 0:
                        ev.append((s, "cancel"))
                part[l] = (a + b) % O.R
            s //= 2
        return ev, part[0]

    def count(ev, where, kind):
        return sum(1 for e in ev if e == (where, kind))

    ev, tot = replay(lay["all_equal_n128"])
    assert count(ev, "lane", "dbl") == 64 and all(count(ev, s, "dbl") == s for s in (32, 16, 8, 4, 2, 1))
    ev, tot = replay(lay["halves_opposite_level32"])
    assert count(ev, 32, "cancel") == 32 and tot == 0
    ev, tot = replay(lay["every_lane_cancels"])
    assert count(ev, "lane", "cancel") == 64 and tot == 0 and len(ev) == 64
    ev, tot = replay(lay["pair_in_one_lane"])
    assert count(ev, "lane", "cancel") == 1 and tot != 0
    ev, tot = replay(lay["pair_in_sibling_lanes"])
    assert count(ev, 32, "cancel") == 1 and tot != 0
    ev, tot = replay(lay["64_cancel_pairwise_then_65th"])
    assert tot == ge.table_sk(17)
    ev, tot = replay(lay["P16_negP16_Q32_dbl_levels_8_4_2_1"])
    assert [count(ev, s, "dbl") for s in (8, 4, 2, 1)] == [8, 4, 2, 1] and count(ev, 32, "dbl") == 0
    ev, tot = replay(lay["P16_negP16_cancel_level16"])
    assert count(ev, 16, "cancel") == 16 and tot == 0
    ev, tot = replay(lay["P16_P16_dbl_level16"])
    assert count(ev, 16, "dbl") == 16
    ev, tot = replay(lay["P8_negP8_cancel_level8"])
    assert count(ev, 8, "cancel") == 8 and tot == 0 and len(lay["P8_negP8_cancel_level8"]) == ge.AGG_MIN
    ev, tot = replay(lay["even_odd_opposite_cancel_level1"])
    assert ev == [(1, "cancel")] and tot == 0
    ev, tot = replay(lay["even_odd_equal_dbl_level1"])
    assert ev == [(1, "dbl")]
    # the cancelling sums serialize as infinity, the continuing ones as the surviving key
    for name in ("halves_opposite_level32", "every_lane_cancels", "P16_negP16_cancel_level16",
                 "P8_negP8_cancel_level8", "even_odd_opposite_cancel_level1", "inf_alone", "inf_x16_whole_list",
                 "inf_lane_then_cancel"):
        assert ge.expected_aggregate(keys, lay[name]) == ge.INF_PK96, name
    raw9 = O.g1_serialize(O.g1_decompress(keys[9])[1])
    assert ge.expected_aggregate(keys, lay["small_a_nega_b"]) == raw9 == ge.expected_aggregate(keys, lay["small_a_b_nega"])
    assert ge.expected_aggregate(keys, lay["64_cancel_pairwise_then_65th"]) == O.g1_serialize(O.g1_decompress(keys[17])[1])
    assert [len(lay["all_equal_n%d" % n]) for n in ge.EQUAL_SIZES] == list(ge.EQUAL_SIZES)
    assert {n for n in ge.EQUAL_SIZES if n < ge.AGG_MIN} and {15, 16, 17, 63, 64, 65} <= set(ge.EQUAL_SIZES)
    rnd = ge.random_pk_lists()
    assert len(rnd) == 40 and {len(r) for r in rnd} >= {1, 15, 16, 17, 64, 65, 130} and max(map(len, rnd)) == 130
    assert {i for r in rnd for i in r} == set(range(8)) | set(range(32, 40))
    assert rnd == ge.random_pk_lists()


def test_low_order_call_positions():
    """the 48-request call puts order-13 and order-23 signatures first, in the middle and
    last in a chunk of 16 and into every slot of a wavefront of 2 and of 3 sets"""
    for pos in (ge.LOW_POS13, ge.LOW_POS23):
        assert {p % 2 for p in pos} == {0, 1} and {p % 3 for p in pos} == {0, 1, 2}
        assert all(0 <= p < ge.LOW_CALL_N for p in pos)
    assert not set(ge.LOW_POS13) & set(ge.LOW_POS23)
    assert {0, 15} <= set(ge.LOW_POS13) and any(0 < p < 15 for p in ge.LOW_POS13)
    assert {31, 47} <= set(ge.LOW_POS23) and any(16 < p < 31 for p in ge.LOW_POS23)
    assert ge.LOW_CALL_N % 16 == 0


def test_expected_worker_restates_expected_stats(oracle):
    """ge.expected_worker is tests/test_gpu_parity.py's _expected_stats (which takes
    single-set batchable requests only) extended to requests of several sets: equal on
    single-set calls"""
    from tests.test_gpu_parity import _expected_stats

    expect = [1] * 16 + [1, 0, 1, -3] + [1] * 12 + [-9] + [1] * 15 + [1] * 16
    want, retries, ok = ge.expected_worker([(True, [t]) for t in expect])
    assert want == expect and (retries, ok) == _expected_stats(oracle, expect) == (2, 32)
    # requests of several sets: a decode error or an infinity key rejects the request, an
    # infinity signature only makes it false
    want, _, _ = ge.expected_worker([(False, [1, -3, 1]), (False, [1, -9, 1]), (False, [-6, 1]), (False, [1, 1]),
                                     (False, [-9])])
    assert want == [-3, 0, -6, 1, -9]


def test_curve_hpp_host_build_on_low_order_points(hostsim, oracle):
    """bls/curve.hpp compiled for the host (tests/native/hostsim.cpp): g2_in_subgroup ->
    jac_mul_xabs on the order-13 points takes jac_add's P == -Q branch, doubles infinity and
    adds to infinity, and must still say 'not in G2'; likewise the order-23 control."""
    import ctypes

    o = ctypes.create_string_buffer(192)
    s13, s23 = ge.low_order_sigs()
    for raw, pt in zip(s13 + s23, ge.q13_multiples() + ge.q23_multiples()):
        assert hostsim.hs_g2_decompress(raw, o) == 0
        (x0, x1), (y0, y1) = pt
        assert o.raw == b"".join(v.to_bytes(48, "big") for v in (x1, x0, y1, y0))
        assert hostsim.hs_g2_in_subgroup(o.raw) == 0


def test_infinity_aggregate_key_is_pk_is_infinity(oracle, golden):
    """The reference's verdict for a set whose aggregate key cancels: BLST_PK_IS_INFINITY,
    alone (core_verify) and among other sets (verifyMultipleSignatures)."""
    O = oracle
    keys = ge.table_keys(golden)
    pts = [O.g1_decompress(keys[i])[1] for i in (1, ge.neg(1))]
    agg = O.aggregate_pubkeys(pts)
    assert agg is None
    sig = bytes.fromhex(golden["signatures"][0]["sig"])
    for sets in ([(agg, _h(b"x"), sig)], [(agg, _h(b"x"), sig), (pts[0], _h(b"y"), sig)]):
        with pytest.raises(O.BlsError) as e:
            O.verify_signature_sets_maybe_batch(sets)
        assert e.value.code == O.E_PK_IS_INFINITY == 6
    # an infinity signature in a request of n >= 2 sets is no error: the batch is just false
    # (verify_multiple skips it in the sum); alone it is ZERO_SIGNATURE
    with pytest.raises(O.BlsError) as e:
        O.verify_signature_sets_maybe_batch([(pts[0], _h(b"x"), ge.INF_SIG96)])
    assert e.value.code == O.E_ZERO_SIGNATURE
