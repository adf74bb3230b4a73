"""Group-law edge cases through every point-summing kernel on cuda:0: P + P, P + (-P) and
infinity as an operand or as a sum (bls/curve.hpp jac_add / jac_add_aff / jac_dbl and the
cooperative programs' zero-checked additions), which the other GPU tests -- distinct keys,
distinct valid signatures, off-group points of huge order -- never reach.

  pubkey aggregation   k_aggregate's serial stage_pk loop (< 16 keys) and the wavefront
                       reduction k_pk_agg (>= 16): runs of equal keys, cancelling halves,
                       lanes and tree levels, a cancelling pair and then more keys, the
                       table's infinity entry; through the verify paths duplicated signers
                       (valid) and a cancelling aggregate (BLST_PK_IS_INFINITY)
  signature sums       k_sig_sum on [s, s], [s, -s], [s, -s, t], infinity members and
                       low-order members
  low-order signatures points of order 13 and 23 on E2 outside G2 through
                       k_g2_decompress, k_sig_decode, both per-set verify paths (k_pset /
                       k_psetn in every wavefront slot, k_chain), k_exact and the
                       same-message path; points of order 3 and 11 on E1 through
                       k_validate_pubkeys.  A point of order 13 makes the [|x|] chain of the
                       subgroup test meet -P, double infinity and add to infinity
                       (tests/_groupedge.py prefix_walk); order 23 is the control that stays
                       on the ordinary branches
  Pippenger / k_gsum   the same signature many times in one pass, also beside its negation
                       and beside an infinity signature

Every expectation is the CPU oracle's: bit-exact bytes, exact codes, verdicts and worker
counters; no tolerance anywhere.  tests/test_groupedge_cpu.py proves the inputs.

The module has its own GpuContext and key table (interop keys 0..31, the negations of keys
0..7 at 32..39, the compressed infinity key at 40); the shared `gpu` fixture's table stays
untouched.  No case was dropped: bls_gpu_load_pubkeys accepts the infinity key with code 0
(asserted by the fixture).

Why the duplicate-signature passes need no fixed seed (test_signature_sum_duplicates*): the
pass's scalars are drawn per call, so which Pippenger buckets collide varies, but a collision
happens in every call.  128 copies of one signature put 128 entries of the same affine point
(and 128 of its mu image) into each 8-bit window's 255 buckets, so every window holds buckets
with several copies (no collision at all has probability about exp(-128^2 / 510) < 1e-13 per
window); at 256 sets a bucket is one segment whose entries k_msm_seg adds in order with mixed
additions, so a bucket that starts with two copies of one point -- a quarter of the ~600
buckets with two or more of the four distinct points -- makes its second msm_madd a doubling.
The check that catches a wrong sum is merged_check == 1: a wrong signature sum fails the
merged pairing and shows as 2.
"""
from __future__ import annotations

import hashlib

import pytest

from lodestar_amd._abi import (
    CODE_PK_IS_INFINITY,
    CODE_POINT_NOT_IN_GROUP,
    DEBUG_MERGED_EVERY_PASS,
    DEBUG_MSM,
    DEBUG_PACK,
    DEBUG_SIGAGG_OFF,
    DEBUG_SIGAGG_ON,
)
from lodestar_amd.native import pack_requests
from tests import _groupedge as ge

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
_PATH_FLAGS = {"pset": DEBUG_SIGAGG_OFF, "sigagg": DEBUG_SIGAGG_ON}


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


class _Edge:
    """the module's context, its table and signatures made on the device"""

    def __init__(self, golden):
        from lodestar_amd.native import GpuContext

        self.ctx = GpuContext(0)
        self.keys = ge.table_keys(golden)
        codes = self.ctx.load_pubkeys(b"".join(self.keys), 48)
        assert list(codes) == [0] * len(self.keys), "load_pubkeys: %s" % list(codes)

    def sign_sk(self, sks, msgs) -> list[bytes]:
        out = self.ctx.sign(b"".join(s.to_bytes(32, "big") for s in sks), b"".join(msgs))
        return [s.tobytes() for s in out]

    def valid_sets(self, tag: bytes, n: int):
        """n valid single-key sets, keys i % 32, distinct roots"""
        msgs = [_h(tag + b"-%d" % i) for i in range(n)]
        sigs = self.sign_sk([ge.table_sk(i % ge.N_BASE) for i in range(n)], msgs)
        return [([i % ge.N_BASE], msgs[i], sigs[i]) for i in range(n)]

    def run(self, pb, path: str, flags: int = 0):
        """one bls_gpu_verify call on the named per-set path with the merged check on
        every pass (nothing is left on the context: no test depends on another's flags)"""
        try:
            self.ctx.set_debug_flags(_PATH_FLAGS[path] | DEBUG_MERGED_EVERY_PASS | flags)
            return self.ctx.verify_packed(pb)
        finally:
            self.ctx.set_debug_flags(0)


@pytest.fixture(scope="module")
def edge(golden):
    e = _Edge(golden)
    yield e
    e.ctx.close()


@pytest.fixture(params=["pset", "sigagg"])
def path(request):
    """both per-set paths (as tests/test_gpu_parity.py's verify_path): the all-cooperative
    k_pset and the aggregated-signature path (k_chain + k_gsum / k_msm + k_mln)"""
    return request.param


# ---------------------------------------------------------------------------
# 2. pubkey aggregation
# ---------------------------------------------------------------------------
_LAYOUTS = ge.pk_layouts()


@pytest.fixture(scope="module")
def pk_agg(edge):
    """every named layout in one bls_gpu_aggregate_pubkeys call: {name: (bytes, code)}"""
    out, codes = edge.ctx.aggregate_pubkeys([lst for _, lst in _LAYOUTS])
    return {name: (o, int(c)) for (name, _), o, c in zip(_LAYOUTS, out, codes)}


@pytest.mark.parametrize("name", [n for n, _ in _LAYOUTS])
def test_aggregate_pubkeys_layout(edge, pk_agg, name):
    """One index list per case (tests/_groupedge.py pk_layouts; lane l of k_pk_agg sums
    positions l, l + 64, ..., tree level s adds lane l + s into lane l):
      all_equal_n*      n copies of one key across the 16-key switch and the 64-lane stride;
                        from n = 65 on lanes double in their own loop, at n = 128 every lane
                        holds 2P and every tree level is a doubling
      halves_opposite   lanes 0..31 P, 32..63 -P: level 32 cancels in every lane
      every_lane_cancels  each lane's second mixed addition gives infinity, the tree adds
                        infinities
      small_a_nega_b / small_a_b_nega   the serial loop: cancel, then continue
      pair_in_one_lane / pair_in_sibling_lanes  a and -a at positions l and l + 64 / l and
                        l + 32 among distinct keys
      64_cancel_pairwise_then_65th  level 32 meets k + key 17 and -k in lane 0, cancels
                        elsewhere
      P16_negP16_Q32    levels 32 and 16 are ordinary (P + Q, -P + Q, then 2Q), levels 8, 4,
                        2 and 1 double equal partial sums
      P16_negP16 / P16_P16   opposite / equal partial sums first meet at level 16
      P8_negP8          opposite partial sums first meet at level 8 (16 keys: the smallest
                        list of the wavefront path)
      even_odd_*        lanes 0 and 1 end as S and -S / as S and S with different Z: the
                        only exceptional addition is the last one, level 1
      inf_*             the table's infinity entry alone, inside lists and as a whole list
                        of 16 (the wavefront path)."""
    lst = dict(_LAYOUTS)[name]
    kernel = "k_pk_agg" if len(lst) >= ge.AGG_MIN else "stage_pk"
    got, code = pk_agg[name]
    want = ge.expected_aggregate(edge.keys, lst)
    assert code == 0, "%s, %s: code %d" % (kernel, name, code)
    assert got == want, "%s, %s: got %s, want %s" % (kernel, name, got.hex(), want.hex())


def test_aggregate_pubkeys_random_lists_with_replacement(edge):
    """40 seeded lists of 1..130 indices drawn with replacement from 8 keys and their
    negations (sync committees are sampled with replacement), one call."""
    lists = ge.random_pk_lists()
    out, codes = edge.ctx.aggregate_pubkeys(lists)
    assert list(codes) == [0] * len(lists)
    for k, (lst, o) in enumerate(zip(lists, out)):
        want = ge.expected_aggregate(edge.keys, lst)
        assert o == want, "random list %d (%d keys): got %s, want %s" % (k, len(lst), o.hex(), want.hex())


def test_verify_duplicated_signers(edge, path):
    """Aggregate sets whose signer lists repeat keys -- [k, k] (serial loop) and a 32-index
    list with 5 repeats (k_pk_agg) -- signed by the matching scalar sum, verify to true,
    alone, batchable and inside one multi-set request."""
    rep32 = list(range(27)) + [3, 3, 11, 20, 26]
    assert len(rep32) == 32 and len(set(rep32)) == 27
    lists = {"[k, k]": [9, 9], "32 with 5 repeats": rep32}
    msgs = {n: _h(b"dup-signers " + n.encode()) for n in lists}
    sigs = dict(zip(lists, edge.sign_sk([ge.list_sk(l) for l in lists.values()], list(msgs.values()))))
    sets = {n: (lists[n], msgs[n], sigs[n]) for n in lists}
    reqs = [(False, [sets[n]]) for n in lists] + [(True, [sets[n]]) for n in lists] + [(False, list(sets.values()))]
    # one signer fewer must fail: the repeated key really counts twice
    short = (rep32[:-1], msgs["32 with 5 repeats"], sigs["32 with 5 repeats"])
    reqs.append((False, [short]))
    v, _ = edge.run(pack_requests(reqs), path)
    assert list(v) == [1, 1, 1, 1, 1, 0], "path %s: %s" % (path, list(v))


def test_verify_cancelling_aggregate_is_pk_infinity(edge, path):
    """A signer list that sums to infinity -- [k, -k] (serial loop) and 32 x k then 32 x -k
    (k_pk_agg) -- is BLST_PK_IS_INFINITY: alone in a non-batchable request, and inside a
    multi-set request next to valid sets (the oracle's core_verify / verify_multiple for
    an infinity key, tests/test_groupedge_cpu.py); the call's other requests keep their
    verdicts."""
    good = edge.valid_sets(b"cancel-neighbours", 4)
    small = ([1, ge.neg(1)], good[0][1], good[0][2])
    big = (dict(_LAYOUTS)["halves_opposite_level32"], good[1][1], good[1][2])
    reqs = [
        ("small alone", False, [small], [-CODE_PK_IS_INFINITY]),
        ("k_pk_agg alone", False, [big], [-CODE_PK_IS_INFINITY]),
        ("valid sets", False, good[:3], [1, 1, 1]),
        ("small among valid", False, [good[0], small, good[1]], [1, -CODE_PK_IS_INFINITY, 1]),
        ("k_pk_agg among valid", False, [good[2], good[3], big], [1, 1, -CODE_PK_IS_INFINITY]),
        ("valid batchable", True, good[3:], [1]),
    ]
    want, _, _ = ge.expected_worker([(b, toks) for _, b, _, toks in reqs])
    assert want == [-6, -6, 1, -6, -6, 1]
    v, _ = edge.run(pack_requests([(b, sets) for _, b, sets, _ in reqs]), path)
    for (name, _, _, _), g, w in zip(reqs, v, want):
        assert g == w, "path %s, %s: verdict %d, want %d" % (path, name, g, w)


# ---------------------------------------------------------------------------
# 3. signature aggregation (k_sig_decode + k_sig_sum)
# ---------------------------------------------------------------------------
_SIG_LISTS = {
    # name: (members, expected code); members name points: s, t, their negations, inf,
    # q13 / q23 (the low-order points)
    "[s, s]": (("s", "s"), 0),
    "[s] * 9": (("s",) * 9, 0),
    "[s, -s]": (("s", "-s"), 0),
    "[s, -s, t]": (("s", "-s", "t"), 0),
    "[s, t, -s]": (("s", "t", "-s"), 0),
    "[inf]": (("inf",), 0),
    "[inf, s]": (("inf", "s"), 0),
    "[s, inf, s]": (("s", "inf", "s"), 0),
    "[s, q13]": (("s", "q13"), CODE_POINT_NOT_IN_GROUP),
    "[q13]": (("q13",), CODE_POINT_NOT_IN_GROUP),
    "[s, q23]": (("s", "q23"), CODE_POINT_NOT_IN_GROUP),
}


@pytest.fixture(scope="module")
def sig_sums(edge):
    s, t = edge.sign_sk([ge.table_sk(2), ge.table_sk(5)], [_h(b"sig-sum s"), _h(b"sig-sum t")])
    s13, s23 = ge.low_order_sigs()
    member = {"s": s, "t": t, "-s": ge.neg_compressed(s), "-t": ge.neg_compressed(t), "inf": ge.INF_SIG96,
              "q13": s13[0], "q23": s23[0]}
    out, codes = edge.ctx.aggregate_signatures([[member[m] for m in ms] for ms, _ in _SIG_LISTS.values()])
    return member, {name: (o, int(c)) for name, o, c in zip(_SIG_LISTS, out, codes)}


@pytest.mark.parametrize("name", list(_SIG_LISTS))
def test_aggregate_signatures_edge_list(sig_sums, oracle, name):
    """k_sig_sum on equal, opposite and infinity members: the compressed sum is the
    oracle's E2.add fold ([s, -s] and [inf] give code 0 and c0 00...); a low-order member
    rejects its list with BLST_POINT_NOT_IN_GROUP."""
    member, res = sig_sums
    members, want_code = _SIG_LISTS[name]
    got, code = res[name]
    assert code == want_code, "k_sig_sum, %s: code %d, want %d" % (name, code, want_code)
    if want_code:
        return
    acc = None
    for m in members:
        acc = oracle.E2.add(acc, oracle.signature_from_bytes(member[m]))
    want = oracle.g2_compress(acc)
    if name in ("[s, -s]", "[inf]"):
        assert want == ge.INF_SIG96
    assert got == want, "k_sig_sum, %s: got %s, want %s" % (name, got.hex(), want.hex())


# ---------------------------------------------------------------------------
# 4. low-order signatures and keys through every decoder and verifier
# ---------------------------------------------------------------------------
_LOW_NAMES = ["order13*%d" % k for k in range(1, 13)] + ["order23*%d" % k for k in (1, 2, 5, 11, 12, 22)]


@pytest.fixture(scope="module")
def low_decoded(edge):
    s13, s23 = ge.low_order_sigs()
    raw = b"".join(s13 + s23)
    return edge.ctx.g2_decompress(raw, validate=True), edge.ctx.g2_decompress(raw, validate=False)


@pytest.mark.parametrize("k", range(len(_LOW_NAMES)), ids=_LOW_NAMES)
def test_g2_decompress_low_order(low_decoded, k):
    """k_g2_decompress on all twelve multiples of the order-13 point and six of the
    order-23 point: validate=True rejects each with BLST_POINT_NOT_IN_GROUP (curve.hpp
    g2_in_subgroup -> jac_mul_xabs on the exceptional branches for order 13);
    validate=False decodes each to the oracle's uncompressed point."""
    (_, codes_v), (out, codes) = low_decoded
    pt = (ge.q13_multiples() + ge.q23_multiples())[k]
    (x0, x1), (y0, y1) = pt
    want = b"".join(v.to_bytes(48, "big") for v in (x1, x0, y1, y0))
    assert codes_v[k] == CODE_POINT_NOT_IN_GROUP, "validate=True, %s: code %d" % (_LOW_NAMES[k], codes_v[k])
    assert codes[k] == 0, "validate=False, %s: code %d" % (_LOW_NAMES[k], codes[k])
    assert out[k].tobytes() == want, "validate=False, %s: got %s" % (_LOW_NAMES[k], out[k].tobytes().hex())


@pytest.fixture(scope="module")
def low_calls(edge):
    """48 single-set batchable requests (three chunks of 16), all valid / with order-23
    signatures only / with order-13 and order-23 signatures at LOW_POS13 and LOW_POS23
    (tests/_groupedge.py): chunk 0's first, a middle and its last request, and every slot
    of a wavefront of 2 and of 3 sets.  {name: (PackedBatch, expected tokens)}"""
    sets = edge.valid_sets(b"low-order-call", ge.LOW_CALL_N)
    s13, s23 = ge.low_order_sigs()
    at13 = {p: s13[(5 * j) % 12] for j, p in enumerate(ge.LOW_POS13)}     # multiples 1, 6, 11, 4, 9
    at23 = {p: s23[j % len(s23)] for j, p in enumerate(ge.LOW_POS23)}
    calls = {}
    for name, subst in (("valid", {}), ("order23", at23), ("order13+23", {**at13, **at23})):
        reqs = [(True, [(pk, m, subst.get(i, sig))]) for i, (pk, m, sig) in enumerate(sets)]
        calls[name] = (pack_requests(reqs), [-CODE_POINT_NOT_IN_GROUP if i in subst else 1
                                             for i in range(ge.LOW_CALL_N)])
    return calls


_PACKINGS = [("auto", 0), ("pack1", DEBUG_PACK(1)), ("pack2", DEBUG_PACK(2)), ("pack3", DEBUG_PACK(3))]


@pytest.mark.parametrize("packing", [p for p, _ in _PACKINGS])
def test_verify_low_order_signatures(edge, path, low_calls, packing):
    """Low-order signatures first, in the middle and last in a chunk of 16 and in every
    slot of a packed wavefront, valid sets around them, on both per-set paths and every
    packing: -BLST_POINT_NOT_IN_GROUP for each low-order set, true for every neighbour,
    the reference's worker counters.

    The zero-check, pinned by the flag count on the cooperative path (k_pset / k_psetn):
    the order-13 signature's [|x|] chain meets -P, so the cooperative addition's zero-check
    must flag the set for k_exact (n_flagged counts at least every order-13 set), whose
    complete formulas then give the verdict; the order-23 sets stay on the ordinary
    branches and must not raise n_flagged above the all-valid call's."""
    flags = dict(_PACKINGS)[packing]
    stats = {}
    for name, (pb, expect) in low_calls.items():
        v, st = edge.run(pb, path, flags)
        want, retries, ok = ge.expected_worker([(True, [t]) for t in expect])
        assert want == expect
        where = "path %s, %s, call %s" % (path, packing, name)
        for i, (g, w) in enumerate(zip(v, expect)):
            assert g == w, "%s: request %d verdict %d, want %d" % (where, i, g, w)
        assert (st.n_chunks, st.batch_retries, st.batch_sigs_success) == (3, retries, ok), where
        assert st.merged_check == (1 if name == "valid" else 2), where
        stats[name] = st
    if path == "pset":
        where = "cooperative path, %s" % packing
        assert stats["order13+23"].n_flagged >= len(ge.LOW_POS13), \
            "%s: n_flagged %d < %d order-13 sets: an exceptional addition went unchecked" % (
                where, stats["order13+23"].n_flagged, len(ge.LOW_POS13))
        assert stats["order23"].n_flagged <= stats["valid"].n_flagged, \
            "%s: order-23 sets flagged (%d, all-valid call %d)" % (
                where, stats["order23"].n_flagged, stats["valid"].n_flagged)


def test_verify_low_order_nonbatchable_and_multiset(edge, path):
    """The low-order signatures outside the chunks: each alone in a non-batchable request
    (the individual pass), and inside multi-set requests (first, last), where the decode
    error of Signature.fromBytes rejects the whole request."""
    good = edge.valid_sets(b"low-order-nb", 4)
    s13, s23 = ge.low_order_sigs()
    q13 = (good[0][0], good[0][1], s13[2])
    q13b = (good[1][0], good[1][1], s13[9])
    q23 = (good[2][0], good[2][1], s23[1])
    reqs = [
        ("order 13 alone", [q13], [-3]),
        ("order 23 alone", [q23], [-3]),
        ("order 13 first of 3", [q13, good[1], good[2]], [-3, 1, 1]),
        ("order 13 last of 3", [good[0], good[2], q13b], [1, 1, -3]),
        ("order 23 in the middle", [good[0], q23, good[3]], [1, -3, 1]),
        ("valid", good, [1, 1, 1, 1]),
    ]
    want, _, _ = ge.expected_worker([(False, toks) for _, _, toks in reqs])
    assert want == [-3, -3, -3, -3, -3, 1]
    v, _ = edge.run(pack_requests([(False, sets) for _, sets, _ in reqs]), path)
    for (name, _, _), g, w in zip(reqs, v, want):
        assert g == w, "path %s, %s: verdict %d, want %d" % (path, name, g, w)


def test_same_message_low_order_signatures(edge):
    """One same-message job of 70 sets (more than one lane round of k_smsum) holding two
    order-13 signatures and one order-23 signature, fixed seed: -3 for those three sets, 1
    for every other."""
    n, msg = 70, _h(b"same-message low order")
    idx = [i % ge.N_BASE for i in range(n)]
    sigs = edge.sign_sk([ge.table_sk(i) for i in idx], [msg] * n)
    s13, s23 = ge.low_order_sigs()
    bad = {3: s13[0], 64: s13[7], 40: s23[3]}
    for p, s in bad.items():
        sigs[p] = s
    got, _ = edge.ctx.verify_same_message([(msg, idx, sigs)], seed=SEED)
    want = [-CODE_POINT_NOT_IN_GROUP if i in bad else 1 for i in range(n)]
    assert len(got) == 1
    for i, (g, w) in enumerate(zip(got[0], want)):
        assert g == w, "same-message job, set %d: verdict %d, want %d" % (i, g, w)


@pytest.mark.parametrize("pk_len", [48, 96])
def test_validate_pubkeys_low_order(edge, oracle, pk_len):
    """k_validate_pubkeys (curve.hpp g1_in_subgroup: two [|x|] chains) on the two order-3
    points (0, +-2) and four points of order 11 on E1, mixed with valid keys: the codes of
    oracle.key_validate, in the 48- and the 96-byte form.  The chains of both orders take
    exceptional additions (tests/_groupedge.py prefix_walk)."""
    ser = oracle.g1_compress if pk_len == 48 else oracle.g1_serialize
    valid = [ser(oracle.g1_decompress(k)[1]) for k in edge.keys[:6]]
    low = [(name, ser(q)) for name, q in ge.low_order_keys()]
    keys, names = [], []
    for j, (name, raw) in enumerate(low):           # valid, low, valid, low, ...
        keys += [valid[j], raw]
        names += ["valid key %d" % j, name]
    want = [oracle.key_validate(k) for k in keys]
    assert want == [0, CODE_POINT_NOT_IN_GROUP] * len(low)
    got = edge.ctx.validate_pubkeys(b"".join(keys), pk_len)
    for name, g, w in zip(names, got, want):
        assert g == w, "k_validate_pubkeys, %d-byte %s: code %d, want %d" % (pk_len, name, g, w)


# ---------------------------------------------------------------------------
# 5. duplicate and opposite points in the Pippenger sum and k_gsum
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def triples(edge):
    """two distinct valid (key, root, signature) triples"""
    msgs = [_h(b"dup triple A"), _h(b"dup triple B")]
    sigs = edge.sign_sk([ge.table_sk(0), ge.table_sk(1)], msgs)
    return ([0], msgs[0], sigs[0]), ([1], msgs[1], sigs[1])


_SUMS = [("k_msm", DEBUG_MSM), ("k_gsum", 0)]


@pytest.mark.parametrize("summer", [s for s, _ in _SUMS])
def test_signature_sum_duplicates(edge, triples, summer):
    """256 single-set batchable requests (16 chunks): two valid triples, each 128 times,
    alternating.  The merged signature sum must pair: merged_check == 1 (2 would be a wrong
    sum).  Under k_msm the Pippenger buckets hold the same affine point several times, so
    k_msm_seg's mixed addition doubles (see the module docstring for why a bucket collision
    happens in every call; a library whose additions never double fails this case).  Under
    k_gsum the summands are [r_i] sig with distinct r_i, distinct points even for equal
    signatures: that run is the same call on the chains' sum, not a doubling in k_gsum."""
    a, b = triples
    pb = pack_requests([(True, [a if i % 2 == 0 else b]) for i in range(256)])
    v, st = edge.run(pb, "sigagg", dict(_SUMS)[summer])
    assert list(v) == [1] * 256, summer
    assert st.merged_check == 1, "%s: merged_check %d: the sum of duplicated signatures is wrong" % (
        summer, st.merged_check)
    assert (st.n_chunks, st.batch_retries, st.batch_sigs_success) == (16, 0, 256), summer
    assert st.pass_shape & 1 == (1 if summer == "k_msm" else 0), summer


@pytest.mark.parametrize("summer", [s for s, _ in _SUMS])
def test_signature_sum_duplicates_and_negations(edge, triples, summer):
    """The same call with the second half of triple A's copies carrying -sig: Pippenger
    buckets hold P and -P together (k_gsum sums [r_i] P and -[r_j] P, opposite only when
    r_i = r_j).  Those 64 sets are invalid; exact verdicts, the
    merged check fails, the worker counters are the reference's (chunks 0..7 pass)."""
    a, b = triples
    neg_a = (a[0], a[1], ge.neg_compressed(a[2]))
    reqs, expect = [], []
    for i in range(256):
        bad = i % 2 == 0 and i >= 128
        reqs.append((True, [neg_a if bad else a if i % 2 == 0 else b]))
        expect.append(0 if bad else 1)
    v, st = edge.run(pack_requests(reqs), "sigagg", dict(_SUMS)[summer])
    want, retries, ok = ge.expected_worker([(True, [t]) for t in expect])
    assert want == expect and (retries, ok) == (8, 128)
    for i, (g, w) in enumerate(zip(v, expect)):
        assert g == w, "%s: request %d verdict %d, want %d" % (summer, i, g, w)
    assert st.merged_check == 2, summer
    assert (st.n_chunks, st.batch_retries, st.batch_sigs_success) == (16, retries, ok), summer


@pytest.mark.parametrize("summer", [s for s, _ in _SUMS])
def test_signature_sum_infinity_signature_beside_duplicates(edge, triples, summer):
    """255 duplicate single-set requests and one multi-set batchable request [A, A, (key,
    root, infinity signature), B]: by the n >= 2 rule of verifyMultipleSignatures the
    request is false with no error code (the oracle skips the infinity signature in the
    sum), every other request is true.  k_msm's msm_point returns the mu image with inf =
    false unconditionally: an infinity signature must never be chain_live."""
    a, b = triples
    inf_set = (a[0], a[1], ge.INF_SIG96)
    reqs = [(True, [a if i % 2 == 0 else b]) for i in range(256)]
    tokens = [(True, [1]) for _ in range(256)]
    reqs[100] = (True, [a, a, inf_set, b])
    tokens[100] = (True, [1, 1, -9, 1])
    want, retries, ok = ge.expected_worker(tokens)
    assert want == [0 if i == 100 else 1 for i in range(256)] and retries == 1
    v, st = edge.run(pack_requests(reqs), "sigagg", dict(_SUMS)[summer])
    for i, (g, w) in enumerate(zip(v, want)):
        assert g == w, "%s: request %d verdict %d, want %d" % (summer, i, g, w)
    assert st.merged_check == 2, summer
    assert (st.n_chunks, st.batch_retries, st.batch_sigs_success) == (16, retries, ok), summer
