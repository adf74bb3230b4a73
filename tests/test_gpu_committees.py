"""Committee-bitfield signature sets on cuda:0: groups registered with
bls_gpu_set_committee_group, sets given as (committee, bits) to
bls_gpu_aggregate_committee_bits and bls_gpu_verify_committees (kernels/k_pk.hip k_pk_bits).

A committee set is exactly the aggregate set whose index list is the committee's members at
the set bits, so every expectation here is that of the expanded list: bit-exact aggregate
bytes against the CPU oracle and against bls_gpu_aggregate_pubkeys, exact codes, and the
verdicts and worker counters of bls_gpu_verify on the expanded twin of the call with the same
seed, which in turn equal the oracle's worker semantics.  No tolerance anywhere.

The module has its own GpuContext and key table: tests/_groupedge.py's 41 entries (interop
keys 0..31, the negations of keys 0..7 -- the keys r - sk -- at 32..39, infinity at 40) and
interop keys 32..99 at 41..108, so 100 distinct keys without a negation serve the committees
of the size sweep and the negations build committees whose total is infinity.

Sizes 1, 7, 8, 9, 63, 64, 65, 129: below, at and above a byte of bits, and below, at and above
the 64 positions one round of the kernel's ballot covers, the last with a third round; the
patterns put the count of set bits on both sides of committee_use_complement's flip
(n - c + 1 < c)."""
from __future__ import annotations

import hashlib
import random

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
    SET_NO_COMMITTEE,
)
from lodestar_amd.native import NativeError, pack_requests
from oracle import bls_oracle as O
from tests import _groupedge as ge

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
SIZES = (1, 7, 8, 9, 63, 64, 65, 129)
EXTRA_BASE = 41  # interop key 32 + j at table index 41 + j, j < 68
POOL = list(range(32)) + list(range(EXTRA_BASE, EXTRA_BASE + 68))  # the 100 distinct interop keys
G_SIZES, G_STRUCT, G_SWAP, G_NEVER = 0, 1, 2, 5

# group G_STRUCT
C_DUP = [5, 9, 5, 12]                                        # member 0 == member 2
C_DUP9 = [5, 9, 5, 12, 13, 14, 15, 16, 17]                   # the same where the complement is taken
C_PAIR = [3, ge.neg(3)]                                      # sk and r - sk: the total is infinity
C_PAIRS6 = [3, ge.neg(3), 4, ge.neg(4), 6, ge.neg(6)]        # the same with room for the complement
STRUCT = [C_DUP, C_DUP9, C_PAIR, C_PAIRS6]


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def _sk(i: int) -> int:
    return O.interop_secret_key(32 + i - EXTRA_BASE) if i >= EXTRA_BASE else ge.table_sk(i)


def _size_committees():
    rng = random.Random(20261020)
    return [rng.sample(POOL, n) if n <= len(POOL) else POOL + rng.sample(POOL, n - len(POOL)) for n in SIZES]


SIZE_COMMITTEES = _size_committees()


def bits_of(n: int, chosen) -> bytes:
    """SSZ order: member j = bit (j & 7) of byte j >> 3"""
    b = bytearray((n + 7) // 8)
    for j in chosen:
        assert 0 <= j < n
        b[j >> 3] |= 1 << (j & 7)
    return bytes(b)


def expand(members, bits: bytes):
    return [m for j, m in enumerate(members) if (bits[j >> 3] >> (j & 7)) & 1]


def patterns(n: int):
    """[(name, positions)] for one size; duplicates among them (n = 1) are kept: every named
    pattern of the sweep runs for every size"""
    h = n // 2
    return [
        ("all", range(n)),
        ("first_only", [0]),
        ("last_only", [n - 1]),
        ("all_but_first", range(1, n)),
        ("all_but_last", range(n - 1)),
        ("half", range(h)),
        ("half_minus_1", range(max(h - 1, 0))),
        ("half_plus_1", range(min(h + 1, n))),
        ("alternating_even", range(0, n, 2)),
        ("alternating_odd", range(1, n, 2)),
    ]


def use_complement(n: int, c: int) -> bool:
    return n - c + 1 < c


class _Ctx:
    def __init__(self, golden):
        from lodestar_amd.native import GpuContext

        self.ctx = GpuContext(0)
        self.keys = ge.table_keys(golden) + [bytes.fromhex(h) for h in golden["kat2_interop_pubkeys"][32:100]]
        assert len(self.keys) == 109 <= 256
        codes = self.ctx.load_pubkeys(b"".join(self.keys), 48)
        assert list(codes) == [0] * len(self.keys)
        self.ctx.set_committee_group(G_SIZES, SIZE_COMMITTEES)
        self.ctx.set_committee_group(G_STRUCT, STRUCT)

    def sign_lists(self, lists, msgs) -> list[bytes]:
        sks = [sum(_sk(i) for i in lst) % O.R for lst in lists]
        out = self.ctx.sign(b"".join(s.to_bytes(32, "big") for s in sks), b"".join(msgs))
        return [s.tobytes() for s in out]

    def expected(self, lst) -> bytes:
        return ge.expected_aggregate(self.keys, lst)


@pytest.fixture(scope="module")
def cm(golden):
    c = _Ctx(golden)
    yield c
    c.ctx.close()


def test_group_info(cm):
    info = cm.ctx.committee_group_info(G_SIZES)
    assert (info["n_committees"], info["n_members"]) == (len(SIZES), sum(SIZES))
    # offsets, members, then 144-byte totals, each part from a 256-byte boundary
    assert info["device_bytes"] == 256 + ((4 * sum(SIZES) + 255) & ~255) + 144 * len(SIZES)
    assert cm.ctx.committee_group_info(G_NEVER) == {"n_committees": 0, "n_members": 0, "device_bytes": 0}
    with pytest.raises(NativeError, match="group 8"):
        cm.ctx.committee_group_info(8)


@pytest.mark.parametrize("k", range(len(SIZES)), ids=["n%d" % n for n in SIZES])
def test_aggregate_parity_size_sweep(cm, k):
    """every pattern of one committee size in one call: bytes == the oracle's aggregate of the
    selected keys == bls_gpu_aggregate_pubkeys of the expanded list; code 0"""
    n, members = SIZES[k], SIZE_COMMITTEES[k]
    pats = patterns(n)
    fields = [bits_of(n, pos) for _, pos in pats]
    lists = [expand(members, f) for f in fields]
    both = {use_complement(n, len(lst)) for lst in lists if lst}
    if n >= 7:
        assert both == {False, True}, "the patterns must take both branches"
    got, codes = cm.ctx.aggregate_committee_bits([((G_SIZES, k), f) for f in fields])
    twin, twin_codes = cm.ctx.aggregate_pubkeys(lists)
    for (name, _), lst, g, c, t, tc in zip(pats, lists, got, codes, twin, twin_codes):
        what = "n=%d %s (c=%d, %s)" % (n, name, len(lst), "complement" if use_complement(n, len(lst)) else "direct")
        assert int(c) == int(tc), what
        if not lst:
            assert int(c) == CODE_EMPTY_AGGREGATE, what  # n = 1: half, half_minus_1, alternating_odd
            continue
        assert int(c) == 0, what
        assert g == cm.expected(lst), what
        assert g == t, what


def test_aggregate_duplicated_member(cm):
    """member 0 == member 2: both bits, one of them, none -- directly (4 members) and where
    the complement is taken (9 members: the total counts the key twice)"""
    cases = []
    for ci, members in ((0, C_DUP), (1, C_DUP9)):
        n = len(members)
        rest = list(range(3, n))
        for name, pos in (("both", [0, 2] + rest), ("first", [0] + rest), ("second", [2] + rest), ("none", [1] + rest),
                          ("both_and_1", [0, 1, 2] + rest), ("only_both", [0, 2])):
            cases.append(("%d members, %s" % (n, name), ci, members, bits_of(n, pos)))
    got, codes = cm.ctx.aggregate_committee_bits([((G_STRUCT, ci), f) for _, ci, _, f in cases])
    lists = [expand(m, f) for _, _, m, f in cases]
    twin, twin_codes = cm.ctx.aggregate_pubkeys(lists)
    assert any(use_complement(9, len(l)) for l in lists) and not all(use_complement(9, len(l)) for l in lists)
    for (name, _, _, _), lst, g, c, t in zip(cases, lists, got, codes, twin):
        assert int(c) == 0, name
        assert g == cm.expected(lst) == t, name


def test_aggregate_cancelling_committee(cm):
    """committees of keys sk and r - sk: the total is infinity.  Every bit set gives the
    infinity aggregate with code 0, as the index list does; all but one member of the
    six-member committee takes the complement, infinity + (-P) = the other's negation"""
    inf96 = O.g1_serialize(None)
    n6 = len(C_PAIRS6)
    cases = [
        ("pair, both", 2, C_PAIR, bits_of(2, [0, 1])),
        ("pair, first", 2, C_PAIR, bits_of(2, [0])),
        ("pair, second", 2, C_PAIR, bits_of(2, [1])),
        ("six, all", 3, C_PAIRS6, bits_of(n6, range(n6))),
        ("six, all but member 0", 3, C_PAIRS6, bits_of(n6, range(1, n6))),
        ("six, all but member 1", 3, C_PAIRS6, bits_of(n6, [0] + list(range(2, n6)))),
        ("six, two pairs", 3, C_PAIRS6, bits_of(n6, [0, 1, 4, 5])),
        ("six, one pair and a key", 3, C_PAIRS6, bits_of(n6, [2, 3, 4])),
    ]
    got, codes = cm.ctx.aggregate_committee_bits([((G_STRUCT, ci), f) for _, ci, _, f in cases])
    lists = [expand(m, f) for _, _, m, f in cases]
    twin, twin_codes = cm.ctx.aggregate_pubkeys(lists)
    res = {}
    for (name, _, _, _), lst, g, c, t, tc in zip(cases, lists, got, codes, twin, twin_codes):
        assert int(c) == int(tc) == 0, name
        assert g == cm.expected(lst) == t, name
        res[name] = g
    assert res["pair, both"] == res["six, all"] == res["six, two pairs"] == inf96
    assert use_complement(n6, n6 - 1)
    # all but key 3 of the six: -(key 3), which is the table's entry 32 + 3
    assert res["six, all but member 0"] == cm.expected([ge.neg(3)])
    assert res["six, all but member 1"] == cm.expected([3])


def test_codes_among_valid_neighbours(cm):
    """each bad set between two good ones in one call; the good ones keep their bytes"""
    n9, m9 = SIZES[3], SIZE_COMMITTEES[3]
    good = bits_of(n9, [0, 3, 8])
    want_good = cm.expected(expand(m9, good))
    bad = [
        ("no bits set", (G_SIZES, 3), bytes(2), CODE_EMPTY_AGGREGATE),
        ("one byte short", (G_SIZES, 3), bytes([0xFF]), CODE_BAD_ENCODING),
        ("one byte long", (G_SIZES, 3), bytes([1, 0, 0]), CODE_BAD_ENCODING),
        ("no bytes", (G_SIZES, 3), b"", CODE_BAD_ENCODING),
        ("padding bit 9 of 9 members", (G_SIZES, 3), bytes([0xFF, 0x03]), CODE_BAD_ENCODING),
        ("padding bit 15 of 9 members", (G_SIZES, 3), bytes([0x01, 0x80]), CODE_BAD_ENCODING),
        ("padding bit 7 of 7 members", (G_SIZES, 1), bytes([0x81]), CODE_BAD_ENCODING),
        ("padding bit 65 of 65 members", (G_SIZES, 6), bytes(8) + bytes([0x02]), CODE_BAD_ENCODING),
        ("unregistered group", (G_NEVER, 0), good, CODE_BAD_ENCODING),
        ("index past the group", (G_SIZES, len(SIZES)), good, CODE_BAD_ENCODING),
        ("index 2^24 - 1", (G_SIZES, 0xFFFFFF), good, CODE_BAD_ENCODING),
        ("group 8 of 8 slots", (8, 0), good, CODE_BAD_ENCODING),
        ("group 254", (254, 0), good, CODE_BAD_ENCODING),
    ]
    sets = [((G_SIZES, 3), good)]
    for _, ref, bits, _ in bad:
        sets += [(ref, bits), ((G_SIZES, 3), good)]
    got, codes = cm.ctx.aggregate_committee_bits(sets)
    for k, (name, _, _, code) in enumerate(bad):
        assert int(codes[2 * k + 1]) == code, name
    for k in range(0, len(sets), 2):
        assert int(codes[k]) == 0 and got[k] == want_good, "neighbour %d" % k
    # the last bit of the last byte that is a member: 64 of 64 members, 8 of 8
    full = cm.ctx.aggregate_committee_bits([((G_SIZES, 5), bytes([0xFF] * 8)), ((G_SIZES, 2), bytes([0x80]))])
    assert list(full[1]) == [0, 0]
    assert full[0][1] == cm.expected([SIZE_COMMITTEES[2][7]])


def test_group_replaced_between_calls(cm):
    """the second call uses the new members and the new totals (the complement reads them);
    a dropped group is unregistered again"""
    old, new = list(range(10, 20)), list(range(41, 56))
    ctx = cm.ctx
    ctx.set_committee_group(G_SWAP, [old])
    f_old = bits_of(10, range(1, 10))  # complement: total - member 0
    got, codes = ctx.aggregate_committee_bits([((G_SWAP, 0), f_old)])
    assert list(codes) == [0] and got[0] == cm.expected(old[1:])
    info_old = ctx.committee_group_info(G_SWAP)
    ctx.set_committee_group(G_SWAP, [new, old])
    info_new = ctx.committee_group_info(G_SWAP)
    assert (info_old["n_committees"], info_old["n_members"]) == (1, 10)
    assert (info_new["n_committees"], info_new["n_members"]) == (2, 25)
    f_new = bits_of(15, range(1, 15))
    got, codes = ctx.aggregate_committee_bits([((G_SWAP, 0), f_new), ((G_SWAP, 1), f_old), ((G_SWAP, 0), f_old)])
    assert list(codes) == [0, 0, 0]
    assert got[0] == cm.expected(new[1:]) and got[1] == cm.expected(old[1:])
    # the old field (2 bytes, bits 1..9) fits the new 15-member committee: its members now
    assert got[2] == cm.expected(new[1:10]) != cm.expected(old[1:])
    ctx.set_committee_group(G_SWAP, [])
    assert ctx.committee_group_info(G_SWAP)["device_bytes"] == 0
    _, codes = ctx.aggregate_committee_bits([((G_SWAP, 0), f_new)])
    assert list(codes) == [CODE_BAD_ENCODING]
    # the other groups were not touched
    got, codes = ctx.aggregate_committee_bits([((G_SIZES, 0), b"\x01")])
    assert list(codes) == [0] and got[0] == cm.expected(SIZE_COMMITTEES[0])


def _mixed_call(cm, bad_batchable: bool):
    """20 requests: (name, batchable, [set...], expected verdict); a set is (kind, list or
    (committee ref, members, bits), message, signature).  Returns the committee form, the
    expanded twin and the expectations."""
    k65, k129, k9, k1 = 6, 7, 3, 0
    m65, m129, m9, m1 = (SIZE_COMMITTEES[k] for k in (k65, k129, k9, k1))
    cset = {
        "c65_two_absent": ((G_SIZES, k65), m65, bits_of(65, [j for j in range(65) if j not in (4, 40)])),
        "c65_three_present": ((G_SIZES, k65), m65, bits_of(65, [0, 33, 64])),
        "c129_five_absent": ((G_SIZES, k129), m129, bits_of(129, [j for j in range(129) if j not in (0, 63, 64, 100, 128)])),
        "c129_half": ((G_SIZES, k129), m129, bits_of(129, range(64))),
        "c9_all": ((G_SIZES, k9), m9, bits_of(9, range(9))),
        "c1": ((G_SIZES, k1), m1, b"\x01"),
        "dup_both": ((G_STRUCT, 1), C_DUP9, bits_of(9, [0, 2, 3, 4, 5, 6, 7, 8])),
        "cancel_all": ((G_STRUCT, 3), C_PAIRS6, bits_of(6, range(6))),
        "empty_bits": ((G_SIZES, k9), m9, bytes(2)),
    }
    lists = {name: expand(m, f) for name, (_, m, f) in cset.items()}
    lists.update({"single_7": [7], "single_50": [50], "single_3": [3], "list_4": [1, 2, 44, 45],
                  "list_20": list(range(41, 61)), "single_9": [9], "single_11": [11]})
    msgs = {name: _h(b"committee-mixed " + name.encode()) for name in lists}
    signed = [n for n in lists if lists[n]]
    sigs = dict(zip(signed, cm.sign_lists([lists[n] for n in signed], [msgs[n] for n in signed])))
    sigs["empty_bits"] = sigs["c9_all"]
    # the cancelling committee's own signature (secret key 0) is the infinity signature, which the
    # one-set rules reject first (ZERO_SIGNATURE); a decodable one lets the key's code show
    sigs["cancel_all"] = sigs["single_7"]
    wrong_msg = _h(b"committee-mixed another root")
    bad_sig = sigs["single_7"]  # a valid signature of another key and root

    # (name, batchable, [(set name, message override, signature override)], verdict)
    plan = [
        ("c65_two_absent", True, [("c65_two_absent", None, None)], 1),
        ("single_7", True, [("single_7", None, None)], 1),
        ("c129_five_absent", True, [("c129_five_absent", None, None)], 1),
        ("list_4", True, [("list_4", None, None)], 1),
        ("c65_three_present", True, [("c65_three_present", None, None)], 1),
        ("block-like: committee, proposer, list", True, [("c129_half", None, None), ("single_50", None, None),
                                                         ("list_20", None, None)], 1),
        ("c9_all", True, [("c9_all", None, None)], 1),
        ("c1", True, [("c1", None, None)], 1),
        ("dup_both", True, [("dup_both", None, None)], 1),
        ("single_3", True, [("single_3", None, None)], 1),
        ("committee, wrong message", bad_batchable, [("c65_two_absent", wrong_msg, None)], 0),
        ("single_9", True, [("single_9", None, None)], 1),
        ("committee, bad signature", bad_batchable, [("c129_five_absent", None, bad_sig)], 0),
        ("single_11", True, [("single_11", None, None)], 1),
        ("c129_half", True, [("c129_half", None, None)], 1),
        ("list_20", True, [("list_20", None, None)], 1),
        ("c65_two_absent again", True, [("c65_two_absent", None, None)], 1),
        # not batchable
        ("committee alone", False, [("c129_five_absent", None, None)], 1),
        ("cancelling committee", False, [("cancel_all", None, None)], -CODE_PK_IS_INFINITY),
        ("no bits set, beside a valid set", False, [("single_7", None, None), ("empty_bits", None, None)],
         -CODE_EMPTY_AGGREGATE),
    ]
    assert len(plan) == 20
    form, twin, tokens = [], [], []
    for _, batchable, sets, verdict in plan:
        a, b = [], []
        for name, m, s in sets:
            m, s = m or msgs[name], s or sigs[name]
            if name in cset:
                (g, i), _, f = cset[name]
                a.append({"committee": (g, i), "bits": f, "message": m, "signature": s})
            else:
                a.append((lists[name], m, s))
            b.append((lists[name], m, s))
        form.append((batchable, a))
        twin.append((batchable, b))
        # the oracle's worker over outcome tokens: a request's sets are valid but for the one
        # its verdict names (ge.expected_worker; -code throws as the aggregation would)
        tokens.append((batchable, [verdict] + [1] * (len(sets) - 1)))
    return form, twin, tokens, [p[3] for p in plan]


@pytest.mark.parametrize("bad", ["bad_in_chunk", "bad_alone"])
@pytest.mark.parametrize("path", ["pset", "sigagg"])
def test_verdict_parity_mixed_call(cm, path, bad):
    """one 20-request call on the per-set path and with BLS_DEBUG_SIGAGG_ON: verdicts and the
    worker counters equal those of bls_gpu_verify on the expanded lists (same seed) and the
    oracle's verify_many_signature_sets.  Fewer than 32 batchable requests are one chunk
    (chunkifyMaximizeChunkSize), so the call runs twice: with the wrong-message set and the bad
    signature inside the chunk, which then fails and is re-verified request by request, and
    with those two requests not batchable, where the chunk of committee sets passes as a
    batch."""
    form, twin, tokens, expect = _mixed_call(cm, bad == "bad_in_chunk")
    pb_c, pb_t = pack_requests(form, seed=SEED), pack_requests(twin, seed=SEED)
    assert pb_c.set_committee is not None and pb_t.set_committee is None
    assert int((pb_c.set_committee != SET_NO_COMMITTEE).sum()) == 14
    flags = {"pset": DEBUG_SIGAGG_OFF, "sigagg": DEBUG_SIGAGG_ON}[path] | DEBUG_MERGED_EVERY_PASS
    try:
        cm.ctx.set_debug_flags(flags)
        v_c, st_c = cm.ctx.verify_committees_packed(pb_c)
        v_t, st_t = cm.ctx.verify_packed(pb_t)
    finally:
        cm.ctx.set_debug_flags(0)
    want, retries, ok = ge.expected_worker(tokens)
    assert want == expect
    # n_chunks and n_individual by the worker's rules (worker.ts:53-98) from the oracle's chunking
    batchable = [(i, t) for i, (b, t) in enumerate(tokens) if b]
    chunks = O.chunkify_maximize_chunk_size(batchable, 16)
    failed = [c for c in chunks if not all(tok == 1 for _, ts in c for tok in ts)]
    n_individual = sum(1 for b, _ in tokens if not b) + sum(len(c) for c in failed)
    assert len(failed) == retries == (1 if bad == "bad_in_chunk" else 0)
    assert (ok > 0) == (bad == "bad_alone")
    counters = lambda st: (st.batch_retries, st.batch_sigs_success, st.n_chunks, st.n_individual)  # noqa: E731
    print("committee form", list(v_c), counters(st_c), "twin", list(v_t), counters(st_t))
    assert list(v_t) == expect, "the expanded twin against the oracle"
    assert list(v_c) == expect
    assert counters(st_t) == (retries, ok, len(chunks), n_individual)
    assert counters(st_c) == counters(st_t)


def test_registration_rejected_keeps_the_group(cm):
    """an index past the table: -2, the message names the committee, and the group's previous
    content still aggregates and verifies"""
    ctx = cm.ctx
    before = ctx.committee_group_info(G_SIZES)
    offs = np.array([0, 2, 5], dtype=np.uint32)
    mem = np.array([0, 1, 2, len(cm.keys), 3], dtype=np.uint32)
    rc = ctx.lib.bls_gpu_set_committee_group(ctx._h, G_SIZES, 2, offs.ctypes.data, mem.ctypes.data)
    assert rc == -2
    msg = ctx.lib.bls_gpu_last_error(ctx._h).decode()
    assert "committee 1" in msg and "table index %d" % len(cm.keys) in msg, msg
    with pytest.raises(NativeError, match="committee 0 is empty"):
        ctx.set_committee_group(G_SIZES, [[], [1]])
    with pytest.raises(NativeError, match="group 8"):
        ctx.set_committee_group(8, [[1]])
    assert ctx.committee_group_info(G_SIZES) == before
    n, members = SIZES[4], SIZE_COMMITTEES[4]
    f = bits_of(n, range(2, n))  # complement: the totals are still the old ones
    lst = expand(members, f)
    got, codes = ctx.aggregate_committee_bits([((G_SIZES, 4), f)])
    assert list(codes) == [0] and got[0] == cm.expected(lst)
    msg32 = _h(b"still verifies")
    sig = cm.sign_lists([lst], [msg32])[0]
    one = {"committee": (G_SIZES, 4), "bits": f, "message": msg32, "signature": sig}
    other = {"committee": (G_SIZES, 4), "bits": bits_of(n, range(3, n)), "message": msg32, "signature": sig}
    v, _ = ctx.verify_committees_packed(pack_requests([(False, [one]), (False, [other])], seed=SEED))
    assert list(v) == [1, 0]


def test_bad_arguments(cm):
    """a raw-pubkey batch, a committee set that also carries an index list, a set without a
    committee that carries bits: -2, nothing run"""
    import ctypes

    from lodestar_amd._abi import BlsStats

    ctx = cm.ctx
    m, s = _h(b"args"), bytes(96)
    raw = pack_requests([(False, [(bytes(96), m, s)])])
    b, _keep = ctx._batch_struct(raw)
    cs, _keep2 = ctx._committee_struct(np.array([COMMITTEE_REF(0, 0)], np.uint32), np.array([0, 1], np.uint32),
                                       np.array([1], np.uint8))
    v = np.zeros(1, np.int32)
    st = BlsStats()
    call = lambda bb, cc: ctx.lib.bls_gpu_verify_committees(ctx._h, ctypes.byref(bb), ctypes.byref(cc),  # noqa: E731
                                                            v.ctypes.data, ctypes.byref(st))
    assert call(b, cs) == -2 and b"set_pk_offsets" in ctx.lib.bls_gpu_last_error(ctx._h)
    tab = pack_requests([(False, [([1], m, s)])])
    b, _keep = ctx._batch_struct(tab)
    assert call(b, cs) == -2 and b"carries an index list" in ctx.lib.bls_gpu_last_error(ctx._h)
    cs2, _keep3 = ctx._committee_struct(np.array([SET_NO_COMMITTEE], np.uint32), np.array([0, 1], np.uint32),
                                        np.array([1], np.uint8))
    assert call(b, cs2) == -2 and b"names no committee" in ctx.lib.bls_gpu_last_error(ctx._h)
    # a batch without any committee set is bls_gpu_verify's
    cs3, _keep4 = ctx._committee_struct(np.array([SET_NO_COMMITTEE], np.uint32), np.array([0, 0], np.uint32),
                                        np.array([0], np.uint8))
    assert call(b, cs3) == 0 and int(v[0]) == -CODE_BAD_ENCODING  # (the all-zero signature)
