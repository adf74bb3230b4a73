"""Span sets through GpuBlsVerifier: a call holding a SpanSet goes out as its own
bls_gpu_verify_spans message -- its CommitteeSets as one-segment spans, its index lists beside
them -- weighs the sum of its segments' 1 + min(c, n - c) keys, and resolves as its expanded
twin does.  On the CPU over the token stand-ins of tests/_standin.py (the host logic alone),
then on cuda:0 with real signatures, two pool contexts and devices = [0, 0]."""
from __future__ import annotations

import hashlib

import pytest

from lodestar_amd._abi import COMMITTEE_REF
from lodestar_amd.verifier import (AGG_KEY_WEIGHT, BlsError, CommitteeSet, GpuBlsVerifier, SignatureSet, SpanSet, _wire,
                                   span_weight_keys)
from tests._spans import concat_bits, span_expand
from tests._standin import INVALID, VALID, TokenCtx


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


class _SpanCtx(TokenCtx):
    """TokenCtx with the committee and span calls: registrations are recorded, both verify
    calls answer over the same validity tokens and record what they were handed"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.groups = {}

    def share_pubkeys(self, other):
        pass

    def set_committee_group(self, group, committees):
        self.groups[group] = [list(c) for c in committees]

    def verify_committees_packed(self, pb):
        assert pb.set_committee is not None and pb.set_span_off is None
        v, st = self.verify_many([pb])
        self.calls[-1] = ("verify_committees", pb.n_sets)
        return v[0], st

    def verify_spans_packed(self, pb):
        assert pb.set_span_off is not None and pb.set_committee is None
        v, st = self.verify_many([pb])
        self.calls[-1] = ("verify_spans", pb.n_sets)
        self.last_span_batch = pb
        return v[0], st


def _verifier(devices, contexts, **kw):
    made = []

    def make(dev, high):
        c = _SpanCtx(dev, high, 0.005)
        made.append(c)
        return c

    return GpuBlsVerifier(devices=devices, n_contexts=contexts, context_factory=make, **kw), made


COMMITTEES = [list(range(0, 9)), list(range(9, 521)), list(range(600, 607))]


def test_span_weight_keys():
    assert span_weight_keys([7, 9], [2, 2]) == 6 and span_weight_keys([512] * 3, [507, 5, 512]) == 6 + 6 + 1


def test_span_call_is_its_own_message_and_weighs_its_segments():
    v, made = _verifier([0, 0], 1)
    try:
        v.set_committee_group(0, COMMITTEES)
        # 7 + 512 + 9 members: 2 of 7 directly; 5 absentees of 512; all of 9
        f = concat_bits([(7, [0, 6]), (512, [j for j in range(512) if j not in (1, 2, 3, 500, 511)]), (9, range(9))])
        span = SpanSet([(0, 2), (0, 1), (0, 0)], f, _h(b"a"), VALID)
        one = CommitteeSet(0, 0, concat_bits([(9, [0, 4])]), _h(b"b"), VALID)
        plain = [SignatureSet(7, _h(b"c"), VALID), SignatureSet(list(range(100, 612)), _h(b"d"), VALID)]
        assert v.verify_signature_sets([span, one] + plain) is True
        assert [k for c in made for k in c.calls] == [("verify_spans", 4)]
        pb = next(c for c in made if c.calls).last_span_batch
        assert list(pb.set_pk_offsets) == [0, 0, 0, 1, 513]
        assert list(pb.set_span_off) == [0, 3, 4, 4, 4]
        assert list(pb.span_refs) == [COMMITTEE_REF(0, 2), COMMITTEE_REF(0, 1), COMMITTEE_REF(0, 0), COMMITTEE_REF(0, 0)]
        assert list(pb.set_bits_off) == [0, 66, 68, 68, 68] and pb.bits.tobytes() == f + one.bits
        # (1 + 2) + (1 + 5) + (1 + 0) keys; 2 of 9 present: 1 + 2 keys; a single key; a 512-key list
        want = (1 + 10 / AGG_KEY_WEIGHT) + (1 + 3 / AGG_KEY_WEIGHT) + 1 + 1.5
        assert sum(s["weight"] for s in v.slot_stats) == pytest.approx(want)
        # without a span the call keeps the committee message; without either, bls_gpu_verify's
        assert v.verify_signature_sets([one] + plain) is True
        assert [k for c in made for k in c.calls][-1] == ("verify_committees", 3)
        assert v.verify_signature_sets(plain) is True
        assert [k for c in made for k in c.calls][-1] == ("verify", 2)
        assert v.verify_signature_sets([SpanSet(span.refs, f, _h(b"a"), INVALID)] + plain) is False
        assert v.verify_signature_sets([span], verify_on_main_thread=True) is True
        assert made[0].calls == [("verify_spans", 1)]
        # batchable jobs of both kinds in one buffer go out as two messages
        futs = [v.verify_signature_sets_async([s], batchable=True) for s in [span, one] + plain]
        assert [x.result(timeout=30) for x in futs] == [True] * 4
        tail = sorted([k for c in made[1:] for k in c.calls][-2:])
        assert tail == [("verify", 2), ("verify_spans", 2)]
    finally:
        v.close()


@pytest.mark.gpu
def test_span_sets_resolve_as_their_expanded_twins(gpu, oracle):
    """real signatures, two pool contexts on devices = [0, 0] and the main-thread lane"""
    n_keys = 48
    sks = [oracle.interop_secret_key(i) for i in range(n_keys)]
    pks = gpu.sk_to_pk(b"".join(s.to_bytes(32, "big") for s in sks)).tobytes()
    committees = [list(range(0, 9)), list(range(9, 42)), [5, 5, 7, 44], list(range(30, 37))]
    groups = {0: committees, 1: committees[::-1]}
    cases = [
        ([(0, 3), (0, 0)], [[0, 6], [0, 8]]),
        ([(0, 0), (0, 1), (1, 0)], [range(1, 9), range(32), [2]]),
        ([(1, 1), (0, 2), (0, 0)], [[0, 1, 3], [1, 2], range(9)]),
        ([(0, 0), (0, 0)], [range(9), range(1, 9)]),
        ([(0, 1), (0, 3)], [[], [6]]),
    ]
    ss, ls = [], []
    for k, (refs, pos) in enumerate(cases):
        mem = [groups[g][i] for g, i in refs]
        bits = concat_bits([(len(m), p) for m, p in zip(mem, pos)])
        lst = span_expand(mem, bits)
        msg = _h(b"verifier-span-%d" % k)
        sig = gpu.sign((sum(sks[i] for i in lst) % oracle.R).to_bytes(32, "big"), msg)[0].tobytes()
        ss.append(SpanSet(refs, bits, msg, sig))
        ls.append(SignatureSet(lst, msg, sig))
    with GpuBlsVerifier(devices=[0, 0], n_contexts=1, pubkeys48=pks) as v:
        ctxs = [v._main] + v._ctxs
        assert len(ctxs) == 3
        for g, cs in groups.items():
            v.set_committee_group(g, cs)
        for batchable in (False, True):
            got = [v.verify_signature_sets_async([s], batchable=batchable) for s in ss]
            twin = [v.verify_signature_sets_async([s], batchable=batchable) for s in ls]
            assert [f.result(timeout=60) for f in got] == [f.result(timeout=60) for f in twin] == [True] * len(ss)
        assert v.verify_signature_sets(ss, verify_on_main_thread=True) is True
        # every context by itself, whichever the routing would have picked
        for c in ctxs:
            verdicts, _ = v._call(c, [(False, [_wire(s)]) for s in ss])
            assert verdicts == [1] * len(ss)
        # a span beside a one-committee set and a single key, one job
        one_bits = concat_bits([(9, [0, 4])])
        one_msg = _h(b"verifier-span-one")
        one_sig = gpu.sign(((sks[0] + sks[4]) % oracle.R).to_bytes(32, "big"), one_msg)[0].tobytes()
        k_msg = _h(b"verifier-span-key")
        k_sig = gpu.sign(sks[40].to_bytes(32, "big"), k_msg)[0].tobytes()
        mixed = [ss[1], CommitteeSet(0, 0, one_bits, one_msg, one_sig), SignatureSet(40, k_msg, k_sig)]
        assert v.verify_signature_sets(mixed) is True
        wrong = SpanSet(ss[0].refs, ss[0].bits, ss[1].signing_root, ss[0].signature)
        assert v.verify_signature_sets([wrong]) is False
        assert v.verify_signature_sets([wrong, ss[1]]) is False
        with pytest.raises(BlsError, match="EMPTY_AGGREGATE_ARRAY"):
            v.verify_signature_sets([SpanSet(ss[0].refs, bytes(2), ss[0].signing_root, ss[0].signature)])
        with pytest.raises(BlsError, match="BLST_BAD_ENCODING"):
            v.verify_signature_sets([SpanSet([(0, 3), (3, 0)], ss[0].bits, ss[0].signing_root, ss[0].signature)])
        # replacing a group changes what a span over it sums
        v.set_committee_group(1, [list(range(20, 27))] + committees[::-1][1:])
        assert v.verify_signature_sets([ss[1]]) is False and v.verify_signature_sets([ss[0]]) is True
