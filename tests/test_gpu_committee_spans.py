"""Span sets on cuda:0: aggregate sets over several registered committees under one field
(EIP-7549 attestations), given to bls_gpu_aggregate_spans and bls_gpu_verify_spans
(kernels/k_pk.hip k_pk_span).

A span set is exactly the aggregate set whose index list is the members of its segments,
concatenated in order, at the set bits, so every expectation is that of the expanded list:
bit-exact aggregate bytes against the CPU oracle and against bls_gpu_aggregate_pubkeys, equal
codes, and the verdicts and worker counters of bls_gpu_verify on the expanded twin of the call
with the same seed, which equal the oracle's worker semantics.  No tolerance anywhere.

The module has its own GpuContext with the 109-key table and the size sweep of
tests/test_gpu_committees.py (tests/_spans.py).  The spans put later segments mid-byte (after
7, 1, 9, 65, 129 members) and mid-way through a round of the kernel's 64-position ballot, reach
the cap of 64 segments, and repeat a committee; the per-segment patterns put each segment's
count on both sides of committee_use_complement's flip, independently of its neighbours."""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np
import pytest

from lodestar_amd._abi import (
    CODE_BAD_ENCODING,
    CODE_EMPTY_AGGREGATE,
    CODE_PK_IS_INFINITY,
    COMMITTEE_REF,
    DEBUG_MERGED_EVERY_PASS,
    DEBUG_SIGAGG_OFF,
    DEBUG_SIGAGG_ON,
    SPAN_MAX_COMMITTEES,
    BlsStats,
)
from lodestar_amd.native import NativeError, pack_requests
from oracle import bls_oracle as O
from tests import _groupedge as ge
from tests import _spans as sp

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))

# the spans of the sweep, by the sizes of their segments
SPANS = {
    "7_9": (7, 9),
    "1_1_1": (1, 1, 1),
    "9_63_65": (9, 63, 65),
    "65_64_1": (65, 64, 1),
    "129_7_129": (129, 7, 129),
    "8_8": (8, 8),
    "cap_64x(1,7)": (1, 7) * (SPAN_MAX_COMMITTEES // 2),
    "9_9_same": (9, 9),
}


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


@pytest.fixture(scope="module")
def cm(golden):
    c = sp.SpanCtx(golden)
    yield c
    c.ctx.close()


def _fields(sizes):
    """[(name, [positions per segment])]: every ordered pair of patterns laid over the segments
    alternately (the pair (p, p) is p everywhere), the seven rotations that give every segment
    another pattern than its neighbours, only the last member of the last segment, and only the
    first member of each segment that starts mid-byte"""
    k = len(sizes)
    out = []
    for p in sp.PATTERNS:
        for q in sp.PATTERNS:
            out.append(("%s/%s" % (p, q), [list(sp.pattern(p if s % 2 == 0 else q, n)) for s, n in enumerate(sizes)]))
    for r in range(len(sp.PATTERNS)):
        out.append(("rot%d" % r, [list(sp.pattern(sp.PATTERNS[(s + r) % len(sp.PATTERNS)], n))
                                  for s, n in enumerate(sizes)]))
    out.append(("last of last", [[] for _ in range(k - 1)] + [[sizes[-1] - 1]]))
    off = 0
    for s, n in enumerate(sizes):
        if off & 7:
            out.append(("first of segment %d at bit %d" % (s, off), [[0] if t == s else [] for t in range(k)]))
        off += n
    return out


@pytest.mark.parametrize("name", list(SPANS))
def test_aggregate_parity_span_sweep(cm, name):
    """every field of one span in one call: bytes == the oracle's aggregate of the expanded
    list == bls_gpu_aggregate_pubkeys of it; codes equal"""
    sizes = SPANS[name]
    refs = [sp.size_ref(n) for n in sizes]
    seg_members = sp.members_of(refs)
    fields = _fields(sizes)
    starts = [sum(sizes[:s]) for s in range(1, len(sizes))]
    assert any(nm.startswith("first of segment") for nm, _ in fields) == any(o & 7 for o in starts)
    assert any(o & 7 for o in starts) or name == "8_8", "but for (8, 8), a later segment starts mid-byte"
    bits = [sp.concat_bits(list(zip(sizes, pos))) for _, pos in fields]
    lists = [sp.span_expand(seg_members, f) for f in bits]
    # both branches, segment by segment and in every combination of two neighbours: over the
    # segments that can take the complement at all (n >= 2; one member never does)
    can = [s for s, n in enumerate(sizes) if n >= 2]
    shapes = {tuple(sp.use_complement(sizes[s], len(pos[s])) for s in can) for _, pos in fields}
    if can:
        assert tuple([False] * len(can)) in shapes and tuple([True] * len(can)) in shapes, "all direct, all complemented"
    if len(can) >= 2:
        firsts = {sh[:2] for sh in shapes}
        assert {(False, True), (True, False)} <= firsts, "(direct, complement) and (complement, direct)"
    got, codes = cm.ctx.aggregate_spans([(refs, f) for f in bits])
    twin, twin_codes = cm.ctx.aggregate_pubkeys(lists)
    n_empty = 0
    for (nm, _), lst, g, c, t, tc in zip(fields, lists, got, codes, twin, twin_codes):
        what = "%s %s (%d of %d keys)" % (name, nm, len(lst), sum(sizes))
        assert int(c) == int(tc), what
        if not lst:
            assert int(c) == CODE_EMPTY_AGGREGATE, what
            n_empty += 1
            continue
        assert int(c) == 0, what
        assert g == cm.expected(lst), what
        assert g == t, what
    assert 1 <= n_empty < len(fields) // 2  # none/none (more for one-member segments), among fields that sum


def test_one_segment_span_is_the_committee_set(cm):
    """a span of one segment: the bytes and codes of bls_gpu_aggregate_committee_bits"""
    sets = []
    for n in sp.SIZES:
        for p in sp.PATTERNS:
            sets.append((sp.size_ref(n), sp.concat_bits([(n, sp.pattern(p, n))])))
    got, codes = cm.ctx.aggregate_spans([([ref], f) for ref, f in sets])
    twin, twin_codes = cm.ctx.aggregate_committee_bits(sets)
    assert list(codes) == list(twin_codes) and got == twin
    assert set(int(c) for c in codes) == {0, CODE_EMPTY_AGGREGATE}


def test_group_law_edges(cm):
    """P + P, P + (-P) and an infinity total, where the kernel meets them: between two totals,
    between two lanes' sums in the tree, and between a sum and a total"""
    inf96 = O.g1_serialize(None)
    nine = sp.size_ref(9)
    m9 = sp.SIZE_COMMITTEES[sp.SIZES.index(9)]
    A, B = (sp.G_STRUCT, sp.S_SHARE_A), (sp.G_STRUCT, sp.S_SHARE_B)
    POS, NEG, PAIR = (sp.G_STRUCT, sp.S_POS), (sp.G_STRUCT, sp.S_NEG), (sp.G_STRUCT, sp.S_PAIR)
    cases = [
        # the repeated committee with every bit set: total + total
        ("same committee twice, all", [nine, nine], [range(9), range(9)]),
        ("same committee three times, all", [nine, nine, nine], [range(9), range(9), range(9)]),
        ("same committee twice, one member each: P + P", [nine, nine], [[4], [4]]),
        ("same committee twice, all but one each", [nine, nine], [range(1, 9), range(1, 9)]),
        # sk and r - sk: the sum is infinity, code 0
        ("pos + neg, all: total + (-total)", [POS, NEG], [range(8), range(8)]),
        ("pos + neg, first only: P + (-P)", [POS, NEG], [[0], [0]]),
        ("pos + neg, all but last: both complemented", [POS, NEG], [range(7), range(7)]),
        ("pos direct + neg complemented", [POS, NEG], [[0, 1], range(8)]),
        ("a total at infinity beside a committee", [PAIR, sp.size_ref(7)], [[0, 1], range(7)]),
        ("a total at infinity alone, twice", [PAIR, PAIR], [[0, 1], [0, 1]]),
        # key 12 in two segments: once directly, once through a complement (total - the rest)
        ("shared key: direct then complement", [A, B], [[2], range(9)]),
        ("shared key: direct then subtracted", [A, B], [[2], [0, 1, 2, 4, 5, 6, 7, 8]]),
        ("shared key: complement then direct", [A, B], [range(9), [3]]),
        ("shared key: subtracted then direct", [A, B], [[0, 1, 3, 4, 5, 6, 7, 8], [3]]),
        ("same committee: member 0 direct, then subtracted", [nine, nine], [[0], range(1, 9)]),
    ]
    sets, lists = [], []
    for _, refs, pos in cases:
        mem = sp.members_of(refs)
        f = sp.concat_bits([(len(m), p) for m, p in zip(mem, pos)])
        sets.append((refs, f))
        lists.append(sp.span_expand(mem, f))
    got, codes = cm.ctx.aggregate_spans(sets)
    twin, twin_codes = cm.ctx.aggregate_pubkeys(lists)
    res = {}
    for (name, _, _), lst, g, c, t, tc in zip(cases, lists, got, codes, twin, twin_codes):
        assert int(c) == int(tc) == 0, name
        assert g == cm.expected(lst), name
        assert g == t, name
        res[name] = g
    for name in ("pos + neg, all: total + (-total)", "pos + neg, first only: P + (-P)",
                 "pos + neg, all but last: both complemented", "a total at infinity alone, twice"):
        assert res[name] == inf96, name
    assert res["same committee twice, one member each: P + P"] == cm.expected([m9[4], m9[4]])
    assert res["shared key: direct then subtracted"] == cm.expected([12] + [m for m in sp.C_SHARE_B if m != 12])
    # the complement branch was the one taken where the case says so
    assert sp.use_complement(9, 8) and sp.use_complement(8, 7) and sp.use_complement(2, 2) and not sp.use_complement(8, 2)


def test_codes_among_valid_neighbours(cm):
    """each bad set between two good ones in one call; the good ones keep their bytes"""
    refs = [sp.size_ref(7), sp.size_ref(9)]  # 16 members, 2 bytes; 9 + 7 + 9 = 25 members: 4 bytes
    refs25 = [sp.size_ref(9), sp.size_ref(7), sp.size_ref(9)]
    good = sp.concat_bits([(7, [0, 6]), (9, [0, 8])])
    want_good = cm.expected(sp.span_expand(sp.members_of(refs), good))
    bad = [
        ("no bit anywhere", refs, bytes(2), CODE_EMPTY_AGGREGATE),
        ("one byte short", refs, bytes([0xFF]), CODE_BAD_ENCODING),
        ("one byte long", refs, bytes([1, 0, 0]), CODE_BAD_ENCODING),
        ("no bytes", refs, b"", CODE_BAD_ENCODING),
        ("one byte short of 25 members", refs25, bytes([1, 0, 0]), CODE_BAD_ENCODING),
        ("padding bit 25 of 25 members", refs25, bytes([1, 0, 0, 0x02]), CODE_BAD_ENCODING),
        ("padding bit 31 of 25 members", refs25, bytes([1, 0, 0, 0x80]), CODE_BAD_ENCODING),
        ("one unregistered segment among registered ones", [sp.size_ref(7), (sp.G_NEVER, 0), sp.size_ref(9)], good,
         CODE_BAD_ENCODING),
        ("an index past its group", [sp.size_ref(7), (sp.G_SIZES, len(sp.SIZES))], good, CODE_BAD_ENCODING),
        ("index 2^24 - 1", [(sp.G_SIZES, 0xFFFFFF), sp.size_ref(9)], good, CODE_BAD_ENCODING),
        ("group 8 of 8 slots", [sp.size_ref(7), (8, 0)], good, CODE_BAD_ENCODING),
        ("group 255", [(255, 0xFFFFFF)], good, CODE_BAD_ENCODING),
    ]
    sets = [(refs, good)]
    for _, r, bits, _ in bad:
        sets += [(r, bits), (refs, good)]
    got, codes = cm.ctx.aggregate_spans(sets)
    for k, (name, _, _, code) in enumerate(bad):
        assert int(codes[2 * k + 1]) == code, name
    for k in range(0, len(sets), 2):
        assert int(codes[k]) == 0 and got[k] == want_good, "neighbour %d" % k
    # the last bit that is a member: bit 24 of 25, and bit 15 of 16 (a full last byte)
    full, fc = cm.ctx.aggregate_spans([(refs25, bytes([0, 0, 0, 0x01])), (refs, bytes([0, 0x80]))])
    assert list(fc) == [0, 0]
    assert full[0] == cm.expected([sp.members_of(refs25)[2][8]]) and full[1] == cm.expected([sp.members_of(refs)[1][8]])
    # a segment with no bit set beside one that has some is legal
    some, sc = cm.ctx.aggregate_spans([(refs, sp.concat_bits([(7, []), (9, [3])]))])
    assert list(sc) == [0] and some[0] == cm.expected([sp.members_of(refs)[1][3]])


def test_too_many_segments_runs_nothing(cm):
    """64 segments are a span; 65 return -2 naming the set, before anything runs"""
    one = sp.size_ref(1)
    f64, f65 = bytes([0xFF] * 8), bytes([0xFF] * 8 + [0x01])
    got, codes = cm.ctx.aggregate_spans([([one] * 64, f64)])
    assert list(codes) == [0] and got[0] == cm.expected(sp.SIZE_COMMITTEES[0] * 64)
    out = np.full(96 * 2, 0xEE, dtype=np.uint8)
    codes = np.full(2, 77, dtype=np.int32)
    ss, _keep = cm.ctx._span_struct(np.array([0, 1, 66], np.uint32), np.array([COMMITTEE_REF(*one)] * 66, np.uint32),
                                    np.array([0, 1, 10], np.uint32), np.frombuffer(b"\x01" + f65, np.uint8))
    rc = cm.ctx.lib.bls_gpu_aggregate_spans(cm.ctx._h, ctypes.byref(ss), 2, out.ctypes.data, codes.ctypes.data)
    assert rc == -2
    msg = cm.ctx.lib.bls_gpu_last_error(cm.ctx._h).decode()
    assert "set 1" in msg and "65 segments" in msg, msg
    assert set(out.tolist()) == {0xEE} and list(codes) == [77, 77], "nothing was written"
    with pytest.raises(NativeError, match="65 segments"):
        cm.ctx.aggregate_spans([([one] * 65, f65)])
    with pytest.raises(NativeError, match="set 0 has no segment"):
        cm.ctx.aggregate_spans([([], b"")])
    assert cm.ctx.aggregate_spans([])[0] == []


def test_bad_arguments(cm):
    """a raw-key batch, a span set that also carries an index list, an index-list set that
    carries bits, offsets that run backwards: -2 with a message naming the set, nothing run"""
    ctx = cm.ctx
    m, s = _h(b"args"), bytes(96)
    v = np.full(1, 55, np.int32)
    st = BlsStats()
    call = lambda bb, ss: ctx.lib.bls_gpu_verify_spans(ctx._h, ctypes.byref(bb), ctypes.byref(ss),  # noqa: E731
                                                       v.ctypes.data, ctypes.byref(st))
    err = lambda: ctx.lib.bls_gpu_last_error(ctx._h)  # noqa: E731
    u32 = lambda *a: np.array(a, np.uint32)  # noqa: E731
    span1, _k0 = ctx._span_struct(u32(0, 1), u32(COMMITTEE_REF(0, 0)), u32(0, 1), np.array([1], np.uint8))
    raw = pack_requests([(False, [(bytes(96), m, s)])])
    b_raw, _k1 = ctx._batch_struct(raw)
    assert call(b_raw, span1) == -2 and b"raw keys" in err()
    tab = pack_requests([(False, [([1], m, s)])])
    b_tab, _k2 = ctx._batch_struct(tab)
    assert call(b_tab, span1) == -2 and b"set 0 is a span and carries an index list" in err()
    lst_bits, _k3 = ctx._span_struct(u32(0, 0), u32(0), u32(0, 1), np.array([1], np.uint8))
    assert call(b_tab, lst_bits) == -2 and b"set 0 has no segment and carries 1 bytes" in err()
    back, _k4 = ctx._span_struct(u32(1, 0), u32(0), u32(0, 0), np.array([1], np.uint8))
    assert call(b_tab, back) == -2 and b"set_span_off[0] != 0" in err()
    assert int(v[0]) == 55
    # a batch without any span is bls_gpu_verify's
    none, _k5 = ctx._span_struct(u32(0, 0), u32(0), u32(0, 0), np.array([0], np.uint8))
    assert call(b_tab, none) == 0 and int(v[0]) == -CODE_BAD_ENCODING  # (the all-zero signature)


def _mixed_call(cm, bad_batchable: bool):
    """20 requests: (name, batchable, [(set name, message override, signature override)],
    expected verdict).  Returns the span form, the expanded twin and the expectations."""
    r = sp.size_ref
    A, B = (sp.G_STRUCT, sp.S_SHARE_A), (sp.G_STRUCT, sp.S_SHARE_B)
    absent = lambda n, gone: [j for j in range(n) if j not in gone]  # noqa: E731
    spans = {  # name: (refs, positions per segment); one ref: a {"committee": ...} dict
        "s_7_9": ([r(7), r(9)], [[0, 6], [0, 8]]),
        "s_65_64_1_absent": ([r(65), r(64), r(1)], [absent(65, (4, 40)), absent(64, (63,)), [0]]),
        "s_129_7_129_mixed": ([r(129), r(7), r(129)], [absent(129, (0, 64, 128)), [], [1, 127]]),
        "s_9_63_65_half": ([r(9), r(63), r(65)], [range(4), range(31), range(32)]),
        "s_cap": ([r(1), r(7)] * 32, [[0], absent(7, (3,))] * 16 + [[], [6]] * 16),
        "s_same_twice": ([r(9), r(9)], [range(9), range(1, 9)]),
        "s_two_groups": ([A, r(8), B], [[2], range(8), absent(9, (3,))]),
        "s_cancel": ([(sp.G_STRUCT, sp.S_POS), (sp.G_STRUCT, sp.S_NEG)], [range(8), range(8)]),
        "s_empty": ([r(7), r(9)], [[], []]),
        "c_65_two_absent": ([r(65)], [absent(65, (4, 40))]),
        "c_9_all": ([r(9)], [range(9)]),
        "c_1": ([r(1)], [[0]]),
    }
    cset, lists = {}, {}
    for name, (refs, pos) in spans.items():
        mem = sp.members_of(refs)
        f = sp.concat_bits([(len(m), p) for m, p in zip(mem, pos)])
        cset[name] = (refs, f)
        lists[name] = sp.span_expand(mem, f)
    lists.update({"single_7": [7], "single_50": [50], "single_3": [3], "list_4": [1, 2, 44, 45],
                  "list_20": list(range(41, 61)), "single_9": [9]})
    msgs = {name: _h(b"span-mixed " + name.encode()) for name in lists}
    signed = [n for n in lists if lists[n]]
    sigs = dict(zip(signed, cm.sign_lists([lists[n] for n in signed], [msgs[n] for n in signed])))
    sigs["s_empty"] = sigs["c_9_all"]
    # the cancelling span's own signature (secret key 0) is the infinity signature, which the
    # one-set rules reject first (ZERO_SIGNATURE); a decodable one lets the key's code show
    sigs["s_cancel"] = sigs["single_7"]
    wrong_msg = _h(b"span-mixed another root")
    bad_sig = sigs["single_7"]  # a valid signature of another key and root

    plan = [
        ("s_7_9", True, [("s_7_9", None, None)], 1),
        ("single_7", True, [("single_7", None, None)], 1),
        ("s_65_64_1_absent", True, [("s_65_64_1_absent", None, None)], 1),
        ("list_4", True, [("list_4", None, None)], 1),
        ("c_65_two_absent", True, [("c_65_two_absent", None, None)], 1),
        ("block-like: span, proposer, list, committee", True, [("s_cap", None, None), ("single_50", None, None),
                                                               ("list_20", None, None), ("c_9_all", None, None)], 1),
        ("s_129_7_129_mixed", True, [("s_129_7_129_mixed", None, None)], 1),
        ("c_1", True, [("c_1", None, None)], 1),
        ("s_same_twice", True, [("s_same_twice", None, None)], 1),
        ("single_3", True, [("single_3", None, None)], 1),
        ("span, wrong message", bad_batchable, [("s_65_64_1_absent", wrong_msg, None)], 0),
        ("single_9", True, [("single_9", None, None)], 1),
        ("span, bad signature", bad_batchable, [("s_129_7_129_mixed", None, bad_sig)], 0),
        ("s_two_groups", True, [("s_two_groups", None, None)], 1),
        ("s_9_63_65_half", True, [("s_9_63_65_half", None, None)], 1),
        ("list_20", True, [("list_20", None, None)], 1),
        ("s_cap", True, [("s_cap", None, None)], 1),
        # not batchable
        ("span alone", False, [("s_9_63_65_half", None, None)], 1),
        ("cancelling span", False, [("s_cancel", None, None)], -CODE_PK_IS_INFINITY),
        ("no bit anywhere, beside a valid set", False, [("single_7", None, None), ("s_empty", None, None)],
         -CODE_EMPTY_AGGREGATE),
    ]
    assert len(plan) == 20
    form, twin, tokens = [], [], []
    for _, batchable, sets, verdict in plan:
        a, b = [], []
        for name, m, s in sets:
            m, s = m or msgs[name], s or sigs[name]
            if name in cset:
                refs, f = cset[name]
                if len(refs) == 1:
                    a.append({"committee": refs[0], "bits": f, "message": m, "signature": s})
                else:
                    a.append({"committees": refs, "bits": f, "message": m, "signature": s})
            else:
                a.append((lists[name], m, s))
            b.append((lists[name], m, s))
        form.append((batchable, a))
        twin.append((batchable, b))
        tokens.append((batchable, [verdict] + [1] * (len(sets) - 1)))
    return form, twin, tokens, [p[3] for p in plan]


@pytest.mark.parametrize("bad", ["bad_in_chunk", "bad_alone"])
@pytest.mark.parametrize("path", ["pset", "sigagg"])
def test_verdict_parity_mixed_call(cm, path, bad):
    """one 20-request call of spans, one-segment spans, index lists and single keys on the
    per-set path and with BLS_DEBUG_SIGAGG_ON: verdicts and the worker counters equal those of
    bls_gpu_verify on the expanded lists (same seed) and the oracle's worker.  Once with the
    wrong-message span and the bad signature inside the chunk, which then fails and is verified
    request by request, and once with those two requests not batchable."""
    form, twin, tokens, expect = _mixed_call(cm, bad == "bad_in_chunk")
    pb_s, pb_t = pack_requests(form, seed=SEED), pack_requests(twin, seed=SEED)
    assert pb_s.set_span_off is not None and pb_s.set_committee is None and pb_t.set_span_off is None
    n_seg = np.diff(pb_s.set_span_off.astype(np.int64))
    assert int((n_seg > 1).sum()) == 13 and int((n_seg == 1).sum()) == 3 and int((n_seg == 0).sum()) == 8
    assert int(n_seg.max()) == SPAN_MAX_COMMITTEES
    flags = {"pset": DEBUG_SIGAGG_OFF, "sigagg": DEBUG_SIGAGG_ON}[path] | DEBUG_MERGED_EVERY_PASS
    try:
        cm.ctx.set_debug_flags(flags)
        v_s, st_s = cm.ctx.verify_spans_packed(pb_s)
        v_t, st_t = cm.ctx.verify_packed(pb_t)
    finally:
        cm.ctx.set_debug_flags(0)
    want, retries, ok = ge.expected_worker(tokens)
    assert want == expect
    batchable = [(i, t) for i, (b, t) in enumerate(tokens) if b]
    chunks = O.chunkify_maximize_chunk_size(batchable, 16)
    failed = [c for c in chunks if not all(tok == 1 for _, ts in c for tok in ts)]
    n_individual = sum(1 for b, _ in tokens if not b) + sum(len(c) for c in failed)
    assert len(failed) == retries == (1 if bad == "bad_in_chunk" else 0)
    assert (ok > 0) == (bad == "bad_alone")
    counters = lambda st: (st.batch_retries, st.batch_sigs_success, st.n_chunks, st.n_individual)  # noqa: E731
    print("span form", list(v_s), counters(st_s), "twin", list(v_t), counters(st_t))
    assert list(v_t) == expect, "the expanded twin against the oracle"
    assert list(v_s) == expect
    assert counters(st_t) == (retries, ok, len(chunks), n_individual)
    assert counters(st_s) == counters(st_t)
    assert (st_s.n_flagged, st_s.n_unique_msgs, st_s.merged_check, st_s.n_ml_units, st_s.pass_shape) == \
           (st_t.n_flagged, st_t.n_unique_msgs, st_t.merged_check, st_t.n_ml_units, st_t.pass_shape)


def test_group_replaced_between_calls(cm):
    """a span over a replaced group sums the new members and, where a segment is complemented,
    reads the new totals; a dropped group makes the span BAD_ENCODING"""
    old, new = list(range(10, 20)), list(range(41, 51))
    ctx = cm.ctx
    nine = sp.size_ref(9)
    m9 = sp.members_of([nine])[0]
    ctx.set_committee_group(sp.G_SWAP, [old])
    refs = [nine, (sp.G_SWAP, 0)]
    f = sp.concat_bits([(9, [0]), (10, range(1, 10))])  # direct, then complement: total - member 0
    got, codes = ctx.aggregate_spans([(refs, f)])
    assert list(codes) == [0] and got[0] == cm.expected([m9[0]] + old[1:])
    ctx.set_committee_group(sp.G_SWAP, [new])
    got2, codes = ctx.aggregate_spans([(refs, f)])
    assert list(codes) == [0] and got2[0] == cm.expected([m9[0]] + new[1:]) != got[0]
    ctx.set_committee_group(sp.G_SWAP, [])
    _, codes = ctx.aggregate_spans([(refs, f), ([nine], bytes([1, 0]))])
    assert list(codes) == [CODE_BAD_ENCODING, 0]
