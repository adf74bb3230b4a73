"""Committee sets through GpuBlsVerifier: set_committee_group reaches every context of every
device and contexts opened later, a call holding a CommitteeSet goes out as its own
bls_gpu_verify_committees message and weighs 1 + min(c, n - c) keys per such set, and it
resolves as its expanded twin does.  On the CPU over the token stand-ins of tests/_standin.py
(the host logic alone), then on cuda:0 with real signatures, two pool contexts and
devices = [0, 0]."""
from __future__ import annotations

import hashlib

import pytest

from lodestar_amd.verifier import (AGG_KEY_WEIGHT, BlsError, CommitteeSet, GpuBlsVerifier, SignatureSet, _wire,
                                   committee_weight_keys)
from tests._standin import INVALID, VALID, TokenCtx


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def _bits(n, chosen) -> bytes:
    b = bytearray((n + 7) // 8)
    for j in chosen:
        b[j >> 3] |= 1 << (j & 7)
    return bytes(b)


class _CommitteeCtx(TokenCtx):
    """TokenCtx with the committee calls: registrations are recorded (and refused for a member
    at or past `table_n`, as the library refuses them), verify_committees_packed answers over
    the same validity tokens and records what it was handed"""

    table_n = 1000

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.groups = {}
        self.shared_with = None

    def share_pubkeys(self, other):
        self.shared_with = other

    def set_committee_group(self, group, committees):
        from lodestar_amd.native import NativeError

        for c, members in enumerate(committees):
            if any(m >= self.table_n for m in members):
                raise NativeError("bls_gpu_set_committee_group: committee group %d: committee %d member past the table"
                                  % (group, c))
        if committees:
            self.groups[group] = [list(c) for c in committees]
        else:
            self.groups.pop(group, None)

    def verify_committees_packed(self, pb):
        assert pb.set_committee is not None
        v, st = self.verify_many([pb])
        self.calls[-1] = ("verify_committees", pb.n_sets)
        self.last_committee_batch = pb
        return v[0], st


def _verifier(devices, contexts, **kw):
    made = []

    def make(dev, high):
        c = _CommitteeCtx(dev, high, 0.005)
        made.append(c)
        return c

    return GpuBlsVerifier(devices=devices, n_contexts=contexts, context_factory=make, **kw), made


COMMITTEES = [list(range(0, 9)), list(range(9, 521))]


def test_committee_weight_keys():
    assert committee_weight_keys(512, 507) == 6 and committee_weight_keys(512, 5) == 6
    assert committee_weight_keys(8, 4) == 5 and committee_weight_keys(1, 1) == 1 and committee_weight_keys(9, 0) == 1


def test_broadcast_reaches_every_context_and_later_ones():
    v, made = _verifier([0, 0], 2)
    try:
        assert len(made) == 5  # the main lane and two contexts per slot
        v.set_committee_group(1, COMMITTEES)
        assert all(c.groups == {1: COMMITTEES} for c in made)
        later = v.add_context(1)
        assert later.groups == {1: COMMITTEES} and later.shared_with is made[0] and len(made) == 6
        assert v._ctx_slot[-1] == 1 and v._slot_ctxs == [2, 3]
        # a rejected registration (the first context decides) changes nothing anywhere
        with pytest.raises(BlsError, match="committee 0"):
            v.set_committee_group(1, [[1, 2, 5000]])
        assert all(c.groups == {1: COMMITTEES} for c in made)
        v.set_committee_group(2, [[3]])
        v.set_committee_group(1, [])
        assert all(c.groups == {2: [[3]]} for c in made)
        assert v.add_context(0).groups == {2: [[3]]}
    finally:
        v.close()


def test_committee_call_is_its_own_message_and_weighs_its_cheaper_form():
    v, made = _verifier([0, 0], 1)
    try:
        v.set_committee_group(0, COMMITTEES)
        absent5 = _bits(512, [j for j in range(512) if j not in (1, 2, 3, 500, 511)])
        cs = [CommitteeSet(0, 1, absent5, _h(b"a"), VALID), CommitteeSet(0, 0, _bits(9, [0, 4]), _h(b"b"), VALID)]
        plain = [SignatureSet(7, _h(b"c"), VALID), SignatureSet(list(range(100, 612)), _h(b"d"), VALID)]
        assert v.verify_signature_sets(cs + plain) is True
        calls = [k for c in made for k in c.calls]
        assert calls == [("verify_committees", 4)]
        pb = next(c for c in made if c.calls).last_committee_batch
        assert list(pb.set_pk_offsets) == [0, 0, 0, 1, 513]
        assert list(pb.set_committee) == [1, 0, 0xFFFFFFFF, 0xFFFFFFFF] and list(pb.set_bits_off) == [0, 64, 66, 66, 66]
        # 5 absentees of 512: 1 + 5 keys; 2 of 9 present: 1 + 2 keys; a single key; a 512-key list
        want = (1 + 6 / AGG_KEY_WEIGHT) + (1 + 3 / AGG_KEY_WEIGHT) + 1 + 1.5
        assert sum(s["weight"] for s in v.slot_stats) == pytest.approx(want)
        # a call without a committee set keeps its message; an invalid committee set fails its call
        assert v.verify_signature_sets(plain) is True
        assert [k for c in made for k in c.calls][-1] == ("verify", 2)
        bad = CommitteeSet(0, 1, absent5, _h(b"a"), INVALID)
        assert v.verify_signature_sets([bad] + plain) is False
        assert v.verify_signature_sets([cs[0]], verify_on_main_thread=True) is True
        assert made[0].calls == [("verify_committees", 1)]
        # batchable jobs of both kinds in one buffer go out as two messages
        futs = [v.verify_signature_sets_async([s], batchable=True) for s in cs + plain]
        assert [f.result(timeout=30) for f in futs] == [True] * 4
        tail = sorted([k for c in made[1:] for k in c.calls][-2:])
        assert tail == [("verify", 2), ("verify_committees", 2)]
    finally:
        v.close()


@pytest.mark.gpu
def test_committee_sets_resolve_as_their_expanded_twins(gpu, oracle):
    """real signatures, two pool contexts on devices = [0, 0] and the main-thread lane"""
    n_keys = 48
    sks = [oracle.interop_secret_key(i) for i in range(n_keys)]
    pks = gpu.sk_to_pk(b"".join(s.to_bytes(32, "big") for s in sks)).tobytes()
    committees = [list(range(0, 9)), list(range(9, 42)), [5, 5, 7, 44]]
    cases = [(0, _bits(9, [0, 1, 2, 3, 4, 5, 6, 8])), (1, _bits(33, [0, 32])), (1, _bits(33, range(1, 33))),
             (2, _bits(4, [0, 1, 3])), (0, _bits(9, [4]))]
    cs, ls = [], []
    for k, (ci, bits) in enumerate(cases):
        lst = [m for j, m in enumerate(committees[ci]) if (bits[j >> 3] >> (j & 7)) & 1]
        msg = _h(b"verifier-committee-%d" % k)
        sig = gpu.sign((sum(sks[i] for i in lst) % oracle.R).to_bytes(32, "big"), msg)[0].tobytes()
        cs.append(CommitteeSet(0, ci, bits, msg, sig))
        ls.append(SignatureSet(lst, msg, sig))
    with GpuBlsVerifier(devices=[0, 0], n_contexts=1, pubkeys48=pks) as v:
        ctxs = [v._main] + v._ctxs
        assert len(ctxs) == 3
        v.set_committee_group(0, committees)
        infos = [c.committee_group_info(0) for c in ctxs]
        assert all((i["n_committees"], i["n_members"]) == (3, 46) for i in infos)
        for batchable in (False, True):
            got = [v.verify_signature_sets_async([s], batchable=batchable) for s in cs]
            twin = [v.verify_signature_sets_async([s], batchable=batchable) for s in ls]
            assert [f.result(timeout=60) for f in got] == [f.result(timeout=60) for f in twin] == [True] * len(cs)
        assert v.verify_signature_sets(cs, verify_on_main_thread=True) is True
        # every context by itself, whichever the routing would have picked
        for c in ctxs:
            verdicts, _ = v._call(c, [(False, [_wire(s)]) for s in cs])
            assert verdicts == [1] * len(cs)
        wrong = CommitteeSet(0, 0, cases[0][1], cs[1].signing_root, cs[0].signature)
        assert v.verify_signature_sets([wrong]) is False
        wrong_twin = SignatureSet(ls[0].pubkey, cs[1].signing_root, cs[0].signature)
        assert v.verify_signature_sets([wrong, cs[1]]) is False and v.verify_signature_sets([wrong_twin, ls[1]]) is False
        with pytest.raises(BlsError, match="EMPTY_AGGREGATE_ARRAY"):
            v.verify_signature_sets([CommitteeSet(0, 0, bytes(2), cs[0].signing_root, cs[0].signature)])
        with pytest.raises(BlsError, match="BLST_BAD_ENCODING"):
            v.verify_signature_sets([CommitteeSet(3, 0, cases[0][1], cs[0].signing_root, cs[0].signature)])
        # a rejected registration changes no context; a context opened later has the group
        with pytest.raises(BlsError, match="committee 0"):
            v.set_committee_group(0, [[0, 1, 1 << 20]])
        assert [c.committee_group_info(0) for c in ctxs] == infos
        later = v.add_context(1)
        assert later.committee_group_info(0) == infos[0]
        assert later.pubkeys_info()["table_id"] == v._main.pubkeys_info()["table_id"]
        assert v._call(later, [(False, [_wire(cs[2])])])[0] == [1]
