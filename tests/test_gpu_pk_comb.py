"""[r] pk on the device table's fixed-base comb rows (bls_gpu_load_pubkeys builds them;
k_chain role 3 and k_pre's per-set-path lanes use them) against the GLV chain, in one
process: two contexts hold the same table, one of them with BLS_DEBUG_NO_PK_COMB.

Expected verdicts and worker counters are the oracle's: every set's outcome is known by
construction (a signature made for the set's key(s) and message, or not), and
oracle.verify_many_signature_sets turns the outcomes into per-request results, batch
retries and successes (the convention of tests/test_gpu_parity.py: the oracle's own
pairings in pure Python take about a second per set)."""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from lodestar_amd._abi import DEBUG_MERGED_EVERY_PASS, DEBUG_NO_PK_COMB, DEBUG_SIGAGG_OFF, DEBUG_SIGAGG_ON
from lodestar_amd.native import GpuContext, pack_requests

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
N1, N2, N3 = 3, 70, 1100  # keys per load: the third passes the table's first capacity (1,028 + 1/2)
SEED = bytes(range(32, 64))


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def _odd_keys(oracle):
    """96-byte on-curve keys outside G1, not cofactor-cleared: (0, 2), of order 3 (the comb
    builder refuses it), and the first x >= 1 with x^3 + 4 a square (it builds)."""
    out, x = [], 0
    while len(out) < 2:
        y = oracle.fp_sqrt((x ** 3 + 4) % oracle.P)
        if y is not None:
            assert not oracle.g1_in_subgroup((x, y))
            out.append(oracle.g1_serialize((x, y)))
        x += 1
    return out


def _expected(oracle, outcomes):
    """(verdicts, batch_retries, batch_sigs_success) of one worker message of requests
    (batchable, [set outcome 1 / 0, ...]) by oracle.verify_many_signature_sets over the
    outcomes (maybeBatch.ts:16-39: a batch is valid iff every set is)."""
    res, retries, ok = oracle.verify_many_signature_sets(list(outcomes), lambda tokens: all(t == 1 for t in tokens))
    assert all(r[0] == "success" for r in res)
    return [1 if r[1] else 0 for r in res], retries, ok


class Pair:
    """the two contexts and the keys' secrets; `on` uses the comb rows, `off` the GLV chain"""

    def __init__(self, oracle):
        self.sks = [oracle.interop_secret_key(i).to_bytes(32, "big") for i in range(N1 + N2 + N3)]
        self.on, self.off = GpuContext(0), GpuContext(0)
        self.pks = self.on.sk_to_pk(b"".join(self.sks))
        self.grown = False
        self.loaded = 0
        self.load(N1)
        self.load(N2)  # "3 keys then 70": two loads, one capacity
        self.paths(DEBUG_SIGAGG_ON)

    def load(self, n):
        blob = self.pks[self.loaded: self.loaded + n].tobytes()
        for c in (self.on, self.off):
            assert (c.load_pubkeys(blob, 48) == 0).all()
        self.loaded += n

    def paths(self, path_flag):
        self.on.base_debug_flags = path_flag | DEBUG_MERGED_EVERY_PASS
        self.off.base_debug_flags = path_flag | DEBUG_MERGED_EVERY_PASS | DEBUG_NO_PK_COMB
        for c in (self.on, self.off):
            c.set_debug_flags(0)

    def sets(self, keys, tag):
        """one valid single-key set per table index in keys"""
        msgs = [_h(tag + b"%d" % i) for i in range(len(keys))]
        sigs = self.on.sign(b"".join(self.sks[k] for k in keys), b"".join(msgs))
        return [([k], m, s.tobytes()) for k, m, s in zip(keys, msgs, sigs)]

    def close(self):
        self.on.close()
        self.off.close()


@pytest.fixture(scope="module")
def pair(oracle):
    p = Pair(oracle)
    yield p
    p.close()


def _call65(pair, keys):
    """65 sets (two wavefronts per role, the second with one lane): single-key sets, key
    keys[5] used by sets 5 and 6, set 10 a 2-key aggregate, set 40 signed for another message"""
    keys = list(keys)
    keys[6] = keys[5]
    sets = pair.sets(keys, b"comb65-")
    a, b = keys[10], keys[11]
    two = pair.on.sign(pair.sks[a] + pair.sks[b], sets[10][1] * 2)
    agg, codes = pair.on.aggregate_signatures([[two[0].tobytes(), two[1].tobytes()]])
    assert codes[0] == 0
    sets[10] = ([a, b], sets[10][1], agg[0])
    good = list(sets)
    sets[40] = (sets[40][0], _h(b"another message"), sets[40][2])
    return sets, good[:40] + good[41:]


def _check_both(pair, oracle, sets, outcomes):
    want, retries, ok = _expected(oracle, [(True, [o]) for o in outcomes])
    pb = pack_requests([(True, [s]) for s in sets], seed=SEED)
    got = {name: c.verify_packed(pb) for name, c in (("on", pair.on), ("off", pair.off))}
    for name, (v, st) in got.items():
        assert list(v) == want, name
        assert (st.batch_retries, st.batch_sigs_success) == (retries, ok), name
    assert got["on"][1].n_flagged == got["off"][1].n_flagged


def test_comb_and_glv_agree_on_a_65_set_call(pair, oracle):
    """k_chain role 3, comb against GLV: verdicts and worker counters equal each other and
    the oracle's; without the invalid set the two contexts' bls_gpu_partial records are
    equal byte for byte (k_mlq evaluates its lines at RP made affine)"""
    pair.paths(DEBUG_SIGAGG_ON)
    keys = [0, 1, 2] + list(range(N1, N1 + 62))  # both loads
    sets, good = _call65(pair, keys)
    _check_both(pair, oracle, sets, [0 if i == 40 else 1 for i in range(65)])
    recs = []
    for c in (pair.on, pair.off):
        rec, status, _err, _st = c.partial(pack_requests([(True, good)], seed=SEED), 0)
        assert status == 0
        recs.append(rec)
    assert recs[0] == recs[1]
    assert pair.on.final_check([recs[0]])


def test_rows_survive_a_table_growth(pair, oracle):
    """a third load past the table's capacity reallocates the table and the rows (the built
    ones are copied): a 65-set call over keys of all three loads, and the two keys outside
    G1 loaded last (one the builder refuses), on both contexts"""
    pair.paths(DEBUG_SIGAGG_ON)
    if not pair.grown:
        pair.load(N3)
        for c in (pair.on, pair.off):
            assert (c.load_pubkeys(b"".join(_odd_keys(oracle)), 96) == 0).all()
        pair.grown = True
    n = N1 + N2 + N3
    keys = [0, 2, 3, 72] + list(range(1000, 1057)) + [n - 4, n - 3, n - 2, n - 1]
    sets, _ = _call65(pair, keys)
    # two more sets name the keys outside G1 (indices n, n + 1) with some key's signature
    sets[50] = ([n], sets[50][1], sets[50][2])
    sets[51] = ([n + 1], sets[51][1], sets[51][2])
    _check_both(pair, oracle, sets, [0 if i in (40, 50, 51) else 1 for i in range(65)])


def test_per_set_path_lanes_agree(pair, oracle):
    """k_pre's RP / RG lanes (the per-set path): a 128-set call of 32 non-batchable requests
    of 4 sets, one set of request 7 signed for another message; both contexts, the oracle"""
    pair.paths(DEBUG_SIGAGG_OFF)
    try:
        sets = pair.sets([(5 * i) % (N1 + N2) for i in range(128)], b"perset-")
        sets[30] = (sets[30][0], _h(b"not this one"), sets[30][2])
        reqs = [(False, sets[4 * r: 4 * r + 4]) for r in range(32)]
        want, _, _ = _expected(oracle, [(False, [0 if 4 * r + k == 30 else 1 for k in range(4)]) for r in range(32)])
        assert want == [0 if r == 7 else 1 for r in range(32)]
        pb = pack_requests(reqs, seed=SEED)
        for name, c in (("on", pair.on), ("off", pair.off)):
            v, _st = c.verify_packed(pb)
            assert list(v) == want, name
    finally:
        pair.paths(DEBUG_SIGAGG_ON)


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
from lodestar_amd._abi import DEBUG_MERGED_EVERY_PASS, DEBUG_SIGAGG_ON
from lodestar_amd.native import GpuContext, pack_requests
from oracle import bls_oracle as O
n, odd = int(sys.argv[2]), [bytes.fromhex(h) for h in sys.argv[3:5]]
sks = [O.interop_secret_key(i).to_bytes(32, "big") for i in range(n)]
with GpuContext(0) as g:
    g.base_debug_flags = DEBUG_SIGAGG_ON | DEBUG_MERGED_EVERY_PASS
    g.set_debug_flags(0)
    assert (g.load_pubkeys(g.sk_to_pk(b"".join(sks)).tobytes(), 48) == 0).all()
    assert (g.load_pubkeys(b"".join(odd), 96) == 0).all()
    keys = list(range(n - 65, n))
    msgs = [hashlib.sha256(b"cap-%d" % i).digest() for i in range(65)]
    sigs = g.sign(b"".join(sks[k] for k in keys), b"".join(msgs))
    sets = [([k], m, s.tobytes()) for k, m, s in zip(keys, msgs, sigs)]
    sets[20] = ([n], sets[20][1], sets[20][2])
    sets[45] = ([n + 1], sets[45][1], sets[45][2])
    sets[64] = (sets[64][0], msgs[0], sets[64][2])
    v, st = g.verify_packed(pack_requests([(True, [s]) for s in sets], seed=bytes(32)))
    print(json.dumps({"v": [int(x) for x in v], "retries": st.batch_retries, "ok": st.batch_sigs_success}))
"""


def test_rows_capped_by_env_in_a_child_process(oracle):
    """BLS_PK_COMB_MAX_MB=1 (read at load time): 728 keys get rows (1 MiB / 1,440 B).  760
    keys and the two keys outside G1 are loaded; a 65-set call over keys 695..759 straddles
    the boundary (33 sets on rows, 32 on the GLV chain, in both wavefronts), two sets name
    the keys outside G1 (past the cap: GLV), one set is signed for another message"""
    n = 760
    assert (1 << 20) // 1440 == 728 and n - 65 < 728 < n
    env = dict(os.environ, BLS_PK_COMB_MAX_MB="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), str(n)] + [k.hex() for k in _odd_keys(oracle)],
                         capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    want, retries, ok = _expected(oracle, [(True, [0 if i in (20, 45, 64) else 1]) for i in range(65)])
    assert got["v"] == want
    assert (got["retries"], got["ok"]) == (retries, ok)
