"""The Pippenger signature sum inside the Miller-loop launches (kernels/k_mlq.hip k_mlq_msm
/ k_mlf_msm, bls/msm.hpp) on cuda:0, against the CPU oracle's worker semantics and against
the same call with the sum as launches of its own (BLS_DEBUG_MSM_SERIAL).

Every call runs with BLS_DEBUG_SIGAGG_ON | BLS_DEBUG_MSM; bls_stats.pass_shape says which
form ran (bit 0 the Pippenger sum, bit 1 its stages inside the Miller-loop launches, bits
8-15 the items per f-side lane).  Verdicts, worker counters and merged_check are exact.

Set counts: 32 single-set requests are the smallest merged call (two chunks); 255, 256 and
257 sets are the edges of a wavefront of four items per lane (256 items) and of a 64-lane
block of one item per lane; at 1,024 sets each window's 255 buckets take 2,048 entries,
8 on average with a segment length of 8, so buckets of two segments are certain (no bucket
above 8 entries in a window has probability far below 1e-30).

Inputs: all valid; one wrong signature (a valid signature over another root); one
undecodable and one out-of-subgroup signature (their sets are not chain_live and return
their codes); an infinity signature inside a multi-set request (flagged, finished by the
exact path, the merged check runs again: flagged_redo); a call in which no set is live,
whose sum over nothing is the point at infinity; and cancelling sets under a pinned seed
(tests/_scalarprobe.py): every set live and valid, the sets of one root signed with keys
chosen so that sum rho_i sk_i = 0 over the root, so that every bucket, window and the final
sum add non-trivial points and the signature sum is infinity (virtual set not live, f = 1);
merged_check == 1 then says the virtual set contributed 1 (any other sum fails the merged
pairing: 2).

The merged product's first levels inside k_mlf ($BLS_MLF_WAVE_PROD) are not built, so no
case here switches them.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from lodestar_amd._abi import (
    CODE_BAD_ENCODING,
    CODE_POINT_NOT_IN_GROUP,
    CODE_ZERO_SIGNATURE,
    DEBUG_MERGED_EVERY_PASS,
    DEBUG_MLF_PL,
    DEBUG_MSM,
    DEBUG_MSM_SERIAL,
    DEBUG_NO_UNITS,
    DEBUG_SIGAGG_ON,
)
from lodestar_amd.native import pack_requests
from tests import _groupedge as ge
from tests import _scalarprobe as sp

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BASE = DEBUG_SIGAGG_ON | DEBUG_MSM
SIZES = (32, 255, 256, 257, 1024)
KINDS = ("valid", "wrong", "codes", "infinity")


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


class _Ctx:
    """the module's context and table; n valid single-key sets per size, signed once"""

    def __init__(self, golden):
        from lodestar_amd.native import GpuContext

        self.ctx = GpuContext(0)
        keys = ge.table_keys(golden)
        assert list(self.ctx.load_pubkeys(b"".join(keys), 48)) == [0] * len(keys)
        self.n_keys = len(keys)
        self._sets = {}

    def add_keys(self, sks) -> list[int]:
        """[sk]g1 for every sk, made on the device and appended to the table: their indices"""
        pks = self.ctx.sk_to_pk(b"".join(k.to_bytes(32, "big") for k in sks))
        assert list(self.ctx.load_pubkeys(pks.tobytes(), 48)) == [0] * len(sks)
        first, self.n_keys = self.n_keys, self.n_keys + len(sks)
        return list(range(first, self.n_keys))

    def sets(self, n: int):
        if n not in self._sets:
            msgs = [_h(b"msm-overlap-%d-%d" % (n, i)) for i in range(n)]
            sks = b"".join(ge.table_sk(i % ge.N_BASE).to_bytes(32, "big") for i in range(n))
            sigs = [s.tobytes() for s in self.ctx.sign(sks, b"".join(msgs))]
            self._sets[n] = [([i % ge.N_BASE], msgs[i], sigs[i]) for i in range(n)]
        return self._sets[n]

    def run(self, reqs, flags: int, seed=None):
        try:
            self.ctx.set_debug_flags(flags)
            v, st = self.ctx.verify_packed(pack_requests(reqs, seed=seed))
            return [int(x) for x in v], st
        finally:
            self.ctx.set_debug_flags(0)


@pytest.fixture(scope="module")
def dev(golden):
    c = _Ctx(golden)
    yield c
    c.ctx.close()


def _call(sets, kind: str):
    """(requests, outcome tokens) of one call over the n valid sets"""
    n = len(sets)
    s, tok = list(sets), [1] * n
    if kind == "wrong":
        j = n // 2
        s[j], tok[j] = (s[j][0], s[j][1], s[(j + 1) % n][2]), 0
    elif kind == "codes":
        s[3], tok[3] = (s[3][0], s[3][1], bytes(96)), -CODE_BAD_ENCODING
        s[n - 2], tok[n - 2] = (s[n - 2][0], s[n - 2][1], ge.low_order_sigs()[0][4]), -CODE_POINT_NOT_IN_GROUP
    elif kind == "dead":
        s13, s23 = ge.low_order_sigs()
        low = s13 + s23
        for j in range(n):
            bad, code = (bytes(96), -CODE_BAD_ENCODING) if j % 5 == 0 else (low[j % len(low)], -CODE_POINT_NOT_IN_GROUP)
            s[j], tok[j] = (s[j][0], s[j][1], bad), code
    reqs = [(True, [x]) for x in s]
    toks = [(True, [t]) for t in tok]
    if kind == "infinity":
        # request 5 gets a second set that carries the infinity signature: false without a
        # code (the n >= 2 rule of verifyMultipleSignatures).  The request count stays n (32
        # requests are two chunks, 31 would be one), the call has n + 1 sets
        inf = (s[6][0], s[6][1], ge.INF_SIG96)
        reqs[5] = (True, [s[5], inf])
        toks[5] = (True, [1, -CODE_ZERO_SIGNATURE])
    return reqs, toks


def _check(dev, reqs, toks, flags, pl, overlapped, where, seed=None):
    want, retries, ok = ge.expected_worker(toks)
    v, st = dev.run(reqs, flags, seed)
    assert v == want, "%s: verdicts differ from the oracle's at %s" % (
        where, [i for i, (g, w) in enumerate(zip(v, want)) if g != w][:8])
    assert (st.batch_retries, st.batch_sigs_success) == (retries, ok), where
    assert st.merged_check == (1 if all(x == 1 for x in want) else 2), (where, st.merged_check)
    assert st.pass_shape & 1 == 1, "%s: the pass did not take the Pippenger sum" % where
    assert (st.pass_shape >> 1) & 1 == (1 if overlapped else 0), "%s: pass_shape %#x" % (where, st.pass_shape)
    assert (st.pass_shape >> 8) & 0xFF == pl, "%s: pass_shape %#x" % (where, st.pass_shape)
    return v, st


@pytest.mark.parametrize("pl", [1, 2, 4])
@pytest.mark.parametrize("n", SIZES)
def test_overlapped_sum_matches_oracle_and_serial_form(dev, n, pl):
    """every input kind at every set count and items per lane: oracle verdicts and counters
    in both forms, the same merged_check and n_flagged, and the form pass_shape reports"""
    flags = BASE | DEBUG_MERGED_EVERY_PASS | DEBUG_MLF_PL(pl)
    for kind in KINDS:
        reqs, toks = _call(dev.sets(n), kind)
        where = "n %d, %d per lane, %s" % (n, pl, kind)
        v1, s1 = _check(dev, reqs, toks, flags, pl, True, where + ", overlapped")
        v0, s0 = _check(dev, reqs, toks, flags | DEBUG_MSM_SERIAL, pl, False, where + ", serial")
        assert v1 == v0 and (s1.merged_check, s1.n_flagged, s1.n_chunks) == (s0.merged_check, s0.n_flagged, s0.n_chunks)
        if kind == "infinity":
            assert s1.n_flagged >= 1, where + ": the infinity signature must take the exact path"


def test_pair_shape_keeps_the_serial_form(dev):
    """one item per two f lanes (MLF_PAIR, k_mlf2) has no fused launch: the serial form"""
    reqs, toks = _call(dev.sets(257), "valid")
    _check(dev, reqs, toks, BASE | DEBUG_MERGED_EVERY_PASS | DEBUG_MLF_PL(3), 3, False, "n 257, MLF_PAIR")


@pytest.mark.parametrize("n", [32, 257])
def test_no_live_set_sums_to_infinity(dev, n):
    """every signature undecodable or outside G2: nothing is chain_live, the sum over no
    point is infinity (virtual set not live, f = 1), every request returns its code"""
    reqs, toks = _call(dev.sets(n), "dead")
    for serial in (0, DEBUG_MSM_SERIAL):
        _check(dev, reqs, toks, BASE | DEBUG_MERGED_EVERY_PASS | DEBUG_MLF_PL(2) | serial, 2, not serial,
               "n %d, no live set, serial %d" % (n, serial))


CANCEL_SEED = bytes(range(64, 96))


def _cancelling_groups(n: int):
    """the sets 0 .. n - 1 in groups that share a root: pairs (2k, 2k + 1), and with n odd
    the last three sets as one group"""
    groups = [[i, i + 1] for i in range(0, n - 3, 2)]
    groups.append(list(range(2 * len(groups), n)))
    assert sorted(i for g in groups for i in g) == list(range(n)) and all(len(g) in (2, 3) for g in groups)
    return groups


@pytest.fixture(scope="module")
def cancelling(dev):
    """{n: requests}: n single-set batchable requests, all valid, whose signature sum under
    CANCEL_SEED is the point at infinity.  A group of sets shares one root m and set i signs
    it with sk_i = c_i d prod_{j != i} rho_j (c = (1, -1) for a pair, (1, 1, -2) for three),
    so sum_i rho_i sk_i = 0: the group's sum rho_i sig_i = [0]H(m) = O and so is its sum
    rho_i pk_i, while every single signature is a non-trivial point of G2, valid for its key."""
    out = {}
    for n in (32, 257):
        sks, msgs = [0] * n, [b""] * n
        for k, grp in enumerate(_cancelling_groups(n)):
            rhos = [sp.rho(CANCEL_SEED, i) for i in grp]
            coef = (1, -1) if len(grp) == 2 else (1, 1, -2)
            for pos, i in enumerate(grp):
                sk = coef[pos] * (k + 3)
                for q, r in enumerate(rhos):
                    if q != pos:
                        sk = sk * r % sp.R
                sks[i], msgs[i] = sk % sp.R, _h(b"msm-overlap-cancel-%d-%d" % (n, k))
            assert sum(r * sks[i] for r, i in zip(rhos, grp)) % sp.R == 0 and all(sks[i] for i in grp)
        idx = dev.add_keys(sks)
        sigs = [s.tobytes() for s in dev.ctx.sign(b"".join(k.to_bytes(32, "big") for k in sks), b"".join(msgs))]
        out[n] = [(True, [([idx[i]], msgs[i], sigs[i])]) for i in range(n)]
    return out


@pytest.mark.parametrize("units", ["units", "no_units"])
@pytest.mark.parametrize("pl", [1, 2, 4])
@pytest.mark.parametrize("n", [32, 257])
def test_cancelling_sets_sum_to_infinity(dev, cancelling, n, pl, units):
    """live, valid sets whose weighted signatures cancel: the buckets, windows and the final
    sum add opposite non-trivial points on the device, the virtual set is not live and
    f = 1, so the merged check passes (1) in both forms; with Miller-loop units the groups'
    key sums are infinity too, without them every set runs its own loop"""
    flags = BASE | DEBUG_MERGED_EVERY_PASS | DEBUG_MLF_PL(pl) | (DEBUG_NO_UNITS if units == "no_units" else 0)
    toks = [(True, [1])] * n
    for serial in (0, DEBUG_MSM_SERIAL):
        v, st = _check(dev, cancelling[n], toks, flags | serial, pl, not serial,
                       "n %d, %d per lane, %s, cancelling, serial %d" % (n, pl, units, serial), seed=CANCEL_SEED)
        assert st.merged_check == 1 and st.n_flagged == 0


def test_three_calls_back_to_back_reuse_the_tickets(dev):
    """valid, failing, valid on one context without a pause: the bucket counts and the six
    tickets are back at zero after every pass, also after the failing one"""
    sets = dev.sets(257)
    flags = BASE | DEBUG_MERGED_EVERY_PASS | DEBUG_MLF_PL(4)
    for k, kind in enumerate(("valid", "wrong", "valid", "codes", "valid")):
        reqs, toks = _call(sets, kind)
        _check(dev, reqs, toks, flags, 4, True, "call %d (%s)" % (k, kind))


def test_merged_after_fail_sequence(dev):
    """the sequence of test_gpu_env_paths.py's msm_flip without BLS_DEBUG_MERGED_EVERY_PASS: a
    failing call on the overlapped sum (merged_check 2), then a passing call that checks its
    chunks straight away (3: no merged sum, no MSM), then one back on the overlapped sum (1)"""
    sets = dev.sets(256)
    flags = BASE | DEBUG_MLF_PL(2)
    reqs, toks = _call(sets, "valid")  # whatever ran before: the context's last merged check passed
    _check(dev, reqs, toks, flags | DEBUG_MERGED_EVERY_PASS, 2, True, "reset")
    seen = []
    for kind in ("wrong", "valid", "valid"):
        reqs, toks = _call(sets, kind)
        want, retries, ok = ge.expected_worker(toks)
        v, st = dev.run(reqs, flags)
        assert v == want and (st.batch_retries, st.batch_sigs_success) == (retries, ok), kind
        seen.append((st.merged_check, st.pass_shape & 3))
    assert seen == [(2, 3), (3, 0), (1, 3)], seen


_CHILD = r"""
import hashlib, json, os, sys
sys.path.insert(0, os.environ["REPO"])
from lodestar_amd._abi import DEBUG_MLF_PL, DEBUG_MSM, DEBUG_SIGAGG_ON
from lodestar_amd.native import GpuContext, pack_requests
from tests import _groupedge as ge
with GpuContext(0) as gpu:
    keys = [bytes.fromhex(k) for k in json.loads(sys.stdin.read())]
    assert list(gpu.load_pubkeys(b"".join(keys), 48)) == [0] * len(keys)
    n = 32
    msgs = [hashlib.sha256(b"overlap-env-%d" % i).digest() for i in range(n)]
    sks = b"".join(ge.table_sk(i).to_bytes(32, "big") for i in range(n))
    sigs = [s.tobytes() for s in gpu.sign(sks, b"".join(msgs))]
    gpu.set_debug_flags(DEBUG_SIGAGG_ON | DEBUG_MSM | DEBUG_MLF_PL(2))
    v, st = gpu.verify_packed(pack_requests([(True, [([i], msgs[i], sigs[i])]) for i in range(n)]))
    print(json.dumps({"verdicts": [int(x) for x in v], "shape": st.pass_shape, "merged": st.merged_check}))
"""


def test_env_switch_forces_the_serial_form(golden):
    """$BLS_MSM_OVERLAP=0 is read once when the library loads: a fresh process"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("BLS_")}
    env.update(BLS_MSM_OVERLAP="0", REPO=str(ROOT))
    keys = json.dumps([k.hex() for k in ge.table_keys(golden, with_infinity=False)])
    r = subprocess.run([sys.executable, "-c", _CHILD], input=keys, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["verdicts"] == [1] * 32 and out["merged"] == 1
    assert out["shape"] & 3 == 1 and (out["shape"] >> 8) & 0xFF == 2, hex(out["shape"])
