"""The split Miller loops (kernels/k_mlq.hip: k_mlq, k_mlf) at every sharing shape of the f
side, on the aggregated-signature path forced on: 1, 2 and 4 items per k_mlf lane
(BLS_DEBUG_MLF_PL), for calls of 1, 63, 65 and 130 batchable single-set requests -- below,
at and across the wavefront and the 16-request chunk, with odd tails in every lane
grouping -- the last request's signature invalid.  Verdicts and batch_retries must equal
oracle.verify_many_signature_sets (the worker's chunking and fallback rules over sets whose
crypto outcome is known by construction, as tests/test_gpu_scale.py does)."""
from __future__ import annotations

import hashlib

import pytest

from lodestar_amd._abi import DEBUG_MERGED_EVERY_PASS, DEBUG_MLF_PL, DEBUG_SIGAGG_ON
from lodestar_amd.native import GpuContext, pack_requests

pytestmark = pytest.mark.gpu

N_MAX = 130


@pytest.fixture(scope="module")
def ctx(golden):
    """a context of its own: the 100 interop keys at table indices 0..99"""
    c = GpuContext(0)
    codes = c.load_pubkeys(b"".join(bytes.fromhex(h) for h in golden["kat2_interop_pubkeys"]), 48)
    assert (codes == 0).all()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(ctx, oracle):
    """130 valid single-key sets over distinct messages, and one signature of another
    message (a valid G2 point that verifies nothing here); signed once for the module"""
    sks = [oracle.interop_secret_key(i % 100).to_bytes(32, "big") for i in range(N_MAX + 1)]
    msgs = [hashlib.sha256(b"ml-shapes-%d" % i).digest() for i in range(N_MAX + 1)]
    sigs = ctx.sign(b"".join(sks), b"".join(msgs))
    good = [([i % 100], msgs[i], sigs[i].tobytes()) for i in range(N_MAX)]
    return good, sigs[N_MAX].tobytes()


def _expect(oracle, n):
    def maybe_batch(tokens):  # maybeBatch.ts:16-39 over outcome tokens (1 valid, 0 invalid)
        if len(tokens) == 0:
            raise oracle.BlsError(oracle.E_EMPTY_SET)
        return all(t == 1 for t in tokens)

    reqs = [(True, [1])] * (n - 1) + [(True, [0])]
    res, retries, ok = oracle.verify_many_signature_sets(reqs, maybe_batch)
    assert all(r[0] == "success" for r in res)
    return [1 if r[1] else 0 for r in res], retries, ok


@pytest.mark.parametrize("per_lane", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_ml_shapes(ctx, oracle, sets, n, per_lane):
    good, other_sig = sets
    reqs = [(True, [s]) for s in good[:n - 1]] + [(True, [(good[n - 1][0], good[n - 1][1], other_sig)])]
    ctx.set_debug_flags(DEBUG_SIGAGG_ON | DEBUG_MERGED_EVERY_PASS | DEBUG_MLF_PL(per_lane))
    try:
        v, st = ctx.verify_packed(pack_requests(reqs))
    finally:
        ctx.set_debug_flags(0)
    verdicts, retries, ok = _expect(oracle, n)
    assert [int(x) for x in v] == verdicts
    assert st.batch_retries == retries and st.batch_sigs_success == ok
