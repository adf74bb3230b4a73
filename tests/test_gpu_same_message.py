"""bls_gpu_verify_same_message (IBlsVerifier.verifySignatureSetsSameMessage) on cuda:0.

Expected verdicts come from three sources: by construction (a set signed with its own key
is valid, a tampered one is not), from bls_gpu_verify over the same sets as n one-set
batchable requests (the existing, oracle-checked path: the verdict arrays must be equal in
every case), and from the Python oracle for a handful of the invalid sets."""
from __future__ import annotations

import hashlib
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lodestar_amd._abi import (
    CODE_BAD_ENCODING,
    CODE_POINT_NOT_IN_GROUP,
    CODE_ZERO_SIGNATURE,
    DEBUG_GROUP_TEST,
    DEBUG_NO_MSG_DEDUP,
)
from lodestar_amd.native import GpuContext, NativeError, pack_requests, pack_same_message

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
N_KEYS = 256
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SHAPES = (1, 2, 63, 64, 65, 129)  # the lane-stride and wavefront-tail edges of k_smsum
SEED = bytes(range(32))


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


class _Fixture:
    def __init__(self):
        self.ctx = GpuContext(0)
        self.sks = [int.from_bytes(_h(i.to_bytes(32, "little")), "little") % R_ORDER for i in range(N_KEYS)]
        self.pks48 = self.ctx.sk_to_pk(b"".join(s.to_bytes(32, "big") for s in self.sks)).tobytes()
        assert (self.ctx.load_pubkeys(self.pks48, 48) == 0).all()

    def sign(self, indices, msg: bytes) -> list[bytes]:
        out = self.ctx.sign(b"".join(self.sks[i].to_bytes(32, "big") for i in indices), msg * len(indices))
        return [s.tobytes() for s in out]

    def job(self, tag: bytes, n: int, first: int = 0):
        """a valid job of n sets: keys first, first + 1, .. (mod the table) signing H(tag)"""
        msg = _h(tag)
        idx = [(first + k) % N_KEYS for k in range(n)]
        return (msg, idx, self.sign(idx, msg))

    def wrong(self, index: int, tag: bytes = b"another root") -> bytes:
        """the key's signature over a root the job does not carry"""
        return self.sign([index], _h(tag))[0]

    def one_set_reference(self, jobs) -> list[np.ndarray]:
        """the same sets as one-set batchable requests through bls_gpu_verify"""
        reqs = [(True, [([i], msg, sig)]) for msg, idx, sigs in jobs for i, sig in zip(idx, sigs)]
        v, _ = self.ctx.verify_packed(pack_requests(reqs, seed=SEED))
        out, off = [], 0
        for _, idx, _ in jobs:
            out.append(v[off: off + len(idx)])
            off += len(idx)
        return out

    def check(self, jobs, expect, seed=SEED):
        """verdicts of the new call == expect (by construction) == the one-set path's"""
        got, st = self.ctx.verify_same_message(jobs, seed=seed)
        ref = self.one_set_reference(jobs)
        assert len(got) == len(jobs)
        for j, (g, e, r) in enumerate(zip(got, expect, ref)):
            assert list(g) == list(e), (j, list(g))
            assert list(r) == list(e), ("one-set path", j, list(r))
        return got, st


@pytest.fixture(scope="module")
def sm():
    f = _Fixture()
    yield f
    f.ctx.close()


@pytest.fixture(scope="module")
def shape_jobs(sm):
    """one call with jobs of 1, 2, 63, 64, 65 and 129 sets, all valid (shared, never edited)"""
    first, jobs = 0, []
    for n in SHAPES:
        jobs.append(sm.job(b"shape%d" % n, n, first))
        first += n
    return tuple(jobs)


def test_shapes_all_valid(sm, shape_jobs):
    got, st = sm.check(list(shape_jobs), [[1] * n for n in SHAPES])
    assert [len(g) for g in got] == list(SHAPES)
    assert st.n_chunks == 5 and st.batch_retries == 0 and st.batch_sigs_success == 323 and st.n_ml_units == 5
    assert st.n_unique_msgs == 6 and st.n_individual == 1  # the 1-set job is verified on its own


def test_shared_root_stays_two_batches(sm):
    a = sm.job(b"shared root", 8, 0)
    b = sm.job(b"shared root", 8, 100)
    sigs = list(b[2])
    sigs[3] = sm.wrong(b[1][3])
    b = (b[0], b[1], sigs)
    _, st = sm.check([a, b], [[1] * 8, [1, 1, 1, 0, 1, 1, 1, 1]])
    assert st.n_unique_msgs == 1
    assert st.n_chunks == 2 and st.batch_retries == 1 and st.batch_sigs_success == 8 and st.n_individual == 8


def test_swapped_signatures_need_the_random_scalars(sm, oracle):
    """the plain sum of the job's signatures still verifies against the sum of its keys, so
    the two swapped sets are found only when r_i is really applied per set"""
    msg, idx, sigs = sm.job(b"swapped", 10, 30)
    sigs[2], sigs[5] = sigs[5], sigs[2]
    sm.check([(msg, idx, sigs)], [[1, 1, 0, 1, 1, 0, 1, 1, 1, 1]])
    # the oracle on the two swapped sets and one valid neighbour (3 of its <= 8 sets)
    pks96, codes = sm.ctx.aggregate_pubkeys([[idx[k]] for k in (2, 3, 5)])
    assert list(codes) == [0, 0, 0]
    res, _, _ = oracle.verify_many_signature_sets([(False, [(pk, msg, sigs[k])]) for pk, k in zip(pks96, (2, 3, 5))])
    assert res == [("success", False), ("success", True), ("success", False)]


def test_one_bad_set_in_the_tail(sm, shape_jobs):
    """set 64 of the 65-set job (the 65th lane's stride) and set 128 of the 129-set job"""
    jobs = [(m, list(i), list(s)) for m, i, s in shape_jobs]
    jobs[4][2][64] = sm.wrong(jobs[4][1][64])
    jobs[5][2][128] = sm.wrong(jobs[5][1][128])
    expect = [[1] * n for n in SHAPES]
    expect[4][64] = 0
    expect[5][128] = 0
    _, st = sm.check(jobs, expect)
    assert st.batch_retries == 2 and st.n_chunks == 5 and st.batch_sigs_success == 2 + 63 + 64
    assert st.n_individual == 1 + 65 + 129


@pytest.fixture(scope="module")
def error_job(sm, golden):
    """20 sets: 96 x 0xFF at 3, the infinity signature at 7, an on-curve point outside G2 at
    11 (the golden fixture tests/test_gpu_parity.py uses), a key index past the table at 15"""
    msg, idx, sigs = sm.job(b"errors", 20, 60)
    sigs[3] = b"\xff" * 96
    sigs[7] = b"\xc0" + bytes(95)
    sigs[11] = bytes.fromhex(next(c["bytes"] for c in golden["sig_decode"] if c["name"] == "not_in_group"))
    idx[15] = N_KEYS + 5
    return msg, idx, sigs


def test_error_sets_inside_a_job(sm, error_job, oracle):
    msg, idx, sigs = error_job
    got, _ = sm.ctx.verify_same_message([error_job], seed=SEED)
    ref = sm.one_set_reference([error_job])
    assert list(got[0]) == list(ref[0])
    v = list(got[0])
    assert v[7] == -CODE_ZERO_SIGNATURE and v[11] == -CODE_POINT_NOT_IN_GROUP and v[15] == -CODE_BAD_ENCODING
    assert v[3] < 0
    assert [x for k, x in enumerate(v) if k not in (3, 7, 11, 15)] == [1] * 16
    # the oracle on the three bad signatures (3 more of its <= 8 sets): the same codes
    pks96, _ = sm.ctx.aggregate_pubkeys([[idx[k]] for k in (3, 7, 11)])
    res, _, _ = oracle.verify_many_signature_sets([(False, [(pk, msg, sigs[k])]) for pk, k in zip(pks96, (3, 7, 11))])
    assert [kind for kind, _ in res] == ["error"] * 3
    assert [-e.code for _, e in res] == [v[3], v[7], v[11]]


def test_seed(sm, shape_jobs, error_job):
    jobs = [shape_jobs[1], error_job, shape_jobs[3]]
    runs = [sm.ctx.verify_same_message(jobs, seed=SEED) for _ in range(2)]
    for (a, sa), (b, sb) in [runs]:
        assert [list(x) for x in a] == [list(x) for x in b]
        for f in ("batch_retries", "batch_sigs_success", "n_chunks", "n_individual", "n_unique_msgs", "n_ml_units",
                  "n_flagged"):
            assert getattr(sa, f) == getattr(sb, f), f
    fresh, st = sm.ctx.verify_same_message(jobs, seed=None)
    assert [list(x) for x in fresh] == [list(x) for x in runs[0][0]]
    assert st.n_chunks == 3 and st.batch_retries == 1 and st.batch_sigs_success == 2 + 64


@pytest.mark.parametrize("flag", [DEBUG_NO_MSG_DEDUP, DEBUG_GROUP_TEST])
def test_existing_path_flags_give_identical_verdicts(sm, shape_jobs, error_job, flag):
    jobs = [(m, list(i), list(s)) for m, i, s in shape_jobs] + [error_job]
    jobs[4][2][64] = sm.wrong(jobs[4][1][64])
    plain, _ = sm.ctx.verify_same_message(jobs, seed=SEED)
    sm.ctx.set_debug_flags(flag)
    try:
        flagged, _ = sm.ctx.verify_same_message(jobs, seed=SEED)
    finally:
        sm.ctx.set_debug_flags(0)
    assert [list(x) for x in flagged] == [list(x) for x in plain]
    assert list(plain[4]) == [1] * 64 + [0] and list(plain[5]) == [1] * 129


def test_bad_arguments(sm, shape_jobs):
    ps = pack_same_message([shape_jobs[1], shape_jobs[2]])
    ps.job_set_offsets = np.array([0, 2, 2, 65], dtype=np.uint32)  # an empty job in the middle
    ps.messages = np.concatenate([ps.messages, ps.messages[:32]])
    rc, _, _ = sm.ctx.verify_same_message_packed(ps)
    assert rc == -2
    with pytest.raises(NativeError, match="empty job"):
        sm.ctx.verify_same_message(ps)
    rc, v, _ = sm.ctx.verify_same_message_packed(pack_same_message([]))
    assert rc == 0 and len(v) == 0
    assert sm.ctx.verify_same_message([])[0] == []


# -- the Python verifier -------------------------------------------------------
def test_python_verifier_same_message(sm):
    from lodestar_amd.verifier import GpuBlsVerifier

    msg_a, idx_a, sigs_a = sm.job(b"verifier a", 64, 0)
    sigs_a[40] = sm.wrong(idx_a[40])
    msg_b, idx_b, sigs_b = sm.job(b"verifier b", 33, 128)
    with GpuBlsVerifier(n_contexts=1, pubkeys48=sm.pks48) as v:
        got = v.verify_signature_sets_same_message(list(zip(idx_a, sigs_a)), msg_a)
        assert got == [k != 40 for k in range(64)] and all(isinstance(x, bool) for x in got)
        # two jobs queued together come back separately
        fa = v.verify_signature_sets_same_message_async(list(zip(idx_a, sigs_a)), msg_a)
        fb = v.verify_signature_sets_same_message_async(list(zip(idx_b, sigs_b)), msg_b)
        assert fb.result(timeout=60) == [True] * 33
        assert fa.result(timeout=60) == [k != 40 for k in range(64)]
        # a key that is not a table index goes through the existing path as a one-set request
        raw = sm.ctx.aggregate_pubkeys([[idx_b[0]]])[0][0]
        mixed = [(raw, sigs_b[0]), (idx_b[1], sigs_b[1]), ([idx_b[2]], sigs_b[3])]
        assert v.verify_signature_sets_same_message(mixed, msg_b) == [True, True, False]


# -- Node: the addon's verifySameMessage and the JS verifier ---------------------
NODE = shutil.which("node")
ADDON = ROOT / "lodestar_amd" / "_native" / "lodestar_bls.node"


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or the N-API addon is absent")
def test_js_same_message(sm, tmp_path):
    msg_a, idx_a, sigs_a = sm.job(b"js a", 64, 0)
    sigs_a[40] = sm.wrong(idx_a[40])
    msg_b, idx_b, sigs_b = sm.job(b"js b", 33, 128)
    raw = sm.ctx.aggregate_pubkeys([[idx_b[0]]])[0][0]
    f = tmp_path / "same.json"
    f.write_text(json.dumps({
        "pubkeys48": sm.pks48.hex(),
        "jobs": [{"msg": m.hex(), "idx": i, "sigs": [s.hex() for s in sg]}
                 for m, i, sg in ((msg_a, idx_a, sigs_a), (msg_b, idx_b, sigs_b))],
        "raw96": raw.hex()}))
    out = subprocess.run([NODE, str(ROOT / "integration" / "js" / "sameMessageTest.js"), str(f)], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["addon"] == "function"
    assert r["single"] == [k != 40 for k in range(64)]
    assert r["together"] == [[k != 40 for k in range(64)], [True] * 33]
    assert r["native"]["verdicts"] == [1 if k != 40 else 0 for k in range(64)] + [1] * 33
    assert r["native"]["stats"]["nChunks"] == 2 and r["native"]["stats"]["batchRetries"] == 1
    assert r["mixed"] == [True, True, False]
    assert r["empty"] == []
    assert "-2" in r["emptyJob"] or "empty job" in r["emptyJob"]
