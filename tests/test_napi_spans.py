"""Span sets through the N-API addon (verifySpans, aggregateSpans) and the JS GpuBlsVerifier
under Node (integration/js/spanTest.js): a {type: "committee", committees: [...]} set resolves
as its expanded twin does on the pool, on every context by itself and on the main-thread lane,
beside one-committee sets and single keys; the aggregate keys are those of the expanded lists;
more than 64 segments are refused before anything runs."""
from __future__ import annotations

import hashlib
import json
import shutil
import subprocess
from pathlib import Path

import pytest

from lodestar_amd._abi import CODE_EMPTY_AGGREGATE
from tests._spans import concat_bits, span_expand

ROOT = Path(__file__).resolve().parent.parent
ADDON = ROOT / "lodestar_amd" / "_native" / "lodestar_bls.node"
NODE = shutil.which("node")
N_KEYS = 48
JS = ROOT / "integration" / "js"

pytestmark = pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or the N-API addon is absent")


def test_addon_exports_the_span_functions():
    code = "const a = require(process.argv[1]); console.log(typeof a.verifySpans, typeof a.aggregateSpans)"
    out = subprocess.run([NODE, "-e", code, str(ADDON)], capture_output=True, text=True, timeout=60, check=True)
    assert out.stdout.split() == ["function"] * 2


def test_js_packs_span_sets():
    """packRequests on the CPU: beside a span, a one-committee set is a one-segment span and an
    index list has empty ranges; no setCommittee array then; packSpans for aggregateSpans"""
    code = """
const m = require(process.argv[1]);
const r = Buffer.alloc(32, 1), s = Buffer.alloc(96, 2);
const sp = {type: "committee", committees: [[0, 1], {group: 2, index: 3}, [0, 1]], bits: Buffer.from([0xfe, 0x81, 1]),
            signingRoot: r, signature: s};
const c = {type: "committee", group: 1, index: 3, bits: Buffer.from([5, 1]), signingRoot: r, signature: s};
const a = m.packRequests([{batchable: true, sets: [{pubkeyIndices: [1, 2], signingRoot: r, signature: s}, sp]},
                          {batchable: false, sets: [c, {pubkeyIndices: [4], signingRoot: r, signature: s}]}]);
const b = m.packRequests([{batchable: true, sets: [c]}]);
const g = new Map([[0, [[], new Array(7).fill(0)]], [2, [[], [], [], new Array(9).fill(0)]]]);
const p = m.packSpans([{committees: [[0, 1], [2, 3]], bits: Buffer.from([1, 2])}, {committees: [[7, 0xffffff]], bits: Buffer.from([3])}]);
console.log(JSON.stringify({spo: Array.from(a.setPkOffsets), idx: Array.from(a.pkIndices), sc: a.setCommittee,
  sso: Array.from(a.setSpanOff), refs: Array.from(a.spanRefs), sbo: Array.from(a.setBitsOff), bits: Array.from(a.bits),
  bSpan: b.setSpanOff, bSc: Array.from(b.setCommittee), w: m.setWeight(sp, g), count: m.getAggregatedPubkeysCount([sp]),
  p: {sso: Array.from(p.setSpanOff), refs: Array.from(p.spanRefs), sbo: Array.from(p.setBitsOff), bits: Array.from(p.bits)}}));
"""
    out = subprocess.run([NODE, "-e", code, str(JS / "gpuBlsVerifier.js")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout)
    assert r["spo"] == [0, 2, 2, 2, 3] and r["idx"] == [1, 2, 4] and r["sc"] is None
    assert r["sso"] == [0, 0, 3, 4, 4] and r["refs"] == [1, (2 << 24) | 3, 1, (1 << 24) | 3]
    assert r["sbo"] == [0, 0, 3, 5, 5] and r["bits"] == [0xFE, 0x81, 1, 5, 1]
    assert r["bSpan"] is None and r["bSc"] == [(1 << 24) | 3]
    # 7 + 9 + 7 members under fe 81 01: segment 0 has bits 1..6 (6 of 7: 1 + 1 key), segment 1 bits 7,
    # 8 and 15 (3 of 9: 1 + 3), segment 2 bit 16 (1 of 7: 1 + 1): 8 keys
    assert r["w"] == 1 + 8 / 1024 and r["count"] == 10
    assert r["p"] == {"sso": [0, 2, 3], "refs": [1, (2 << 24) | 3, 0x07FFFFFF], "sbo": [0, 2, 3], "bits": [1, 2, 3]}


@pytest.mark.gpu
def test_js_verifier_span_sets(gpu, oracle, tmp_path):
    sks = [oracle.interop_secret_key(i) for i in range(N_KEYS)]
    pks = gpu.sk_to_pk(b"".join(s.to_bytes(32, "big") for s in sks))
    committees = [list(range(0, 9)), list(range(9, 42)), [5, 5, 7, 44], list(range(30, 37))]
    groups = {0: committees, 1: committees[::-1]}
    cases = [  # (refs, positions per segment)
        ([(0, 3), (0, 0)], [[0, 6], [0, 8]]),                                  # 7 + 9: both direct
        ([(0, 0), (0, 1), (1, 0)], [range(1, 9), range(32), [2]]),             # complement, complement, direct
        ([(0, 1)], [[0, 32]]),                                                 # one segment
        ([(1, 1), (0, 2), (0, 0)], [[0, 1, 3], [1, 2], range(9)]),             # a duplicated member, two groups
        ([(0, 0), (0, 0)], [range(9), range(1, 9)]),                           # the same committee twice
    ]
    sets = []
    for k, (refs, pos) in enumerate(cases):
        mem = [groups[g][i] for g, i in refs]
        bits = concat_bits([(len(m), p) for m, p in zip(mem, pos)])
        lst = span_expand(mem, bits)
        msg = hashlib.sha256(b"napi-span-%d" % k).digest()
        sk = sum(sks[i] for i in lst) % oracle.R
        sig = gpu.sign(sk.to_bytes(32, "big"), msg)[0].tobytes()
        key = gpu.sk_to_pk(sk.to_bytes(32, "big")).tobytes()
        code, pt = oracle.g1_decompress(key)
        assert code == 0
        sets.append({"committees": [list(r) for r in refs], "bits": bits.hex(), "list": lst, "msg": msg.hex(),
                     "sig": sig.hex(), "key96": oracle.g1_serialize(pt).hex()})
    smsgs = [hashlib.sha256(b"napi-span-single-%d" % i).digest() for i in range(3)]
    ssigs = gpu.sign(b"".join(sks[40 + i].to_bytes(32, "big") for i in range(3)), b"".join(smsgs))
    singles = [{"idx": 40 + i, "msg": smsgs[i].hex(), "sig": ssigs[i].tobytes().hex()} for i in range(3)]
    f = tmp_path / "spans.json"
    f.write_text(json.dumps({"keys48": pks.tobytes().hex(), "committees": committees, "sets": sets, "singles": singles}))
    out = subprocess.run([NODE, str(JS / "spanTest.js"), str(f)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["addon"] == ["function"] * 2
    assert r["span"] == r["expanded"] == [True] * len(cases)
    assert r["perContext"] == [[1] * len(cases)] * 3
    assert r["mainLane"] is True and r["mixed"] is True and r["wrong"] is False
    assert "BLST_BAD_ENCODING" in r["unregistered"] and "EMPTY_AGGREGATE_ARRAY" in r["noBits"]
    assert "65 segments" in r["tooMany"] and "65 segments" in r["aggTooMany"]
    # keys per set: sum over segments of 1 + min(c, n - c)
    assert r["weights"] == [1 + 6 / 1024, 1 + 6 / 1024, 1 + 3 / 1024, 1 + 6 / 1024, 1 + 3 / 1024]
    assert r["aggCodes"] == [0] * len(cases) and r["aggKeys"] == [s["key96"] for s in sets]
    assert r["rawCodes"] == [CODE_EMPTY_AGGREGATE, 0] and r["rawKey1"] == sets[0]["key96"]
