"""Failed-chunk recovery on the GPU, swept (tests/_recovery.py): every message of the sweep
through bls_gpu_verify_many, its verdicts and summed worker counters against the oracle's
worker semantics, and the eight round counters of bls_gpu_group_test_counts against the
model of the group-test rounds -- so a complement inference that silently falls through to
one test per request (right verdicts, 16 final exponentiations instead of 5) fails here.

* in process, default knobs, on both per-set paths: the sweep and the request-structure
  list, with the merged check (merged_check 2) and straight after without
  BLS_DEBUG_MERGED_EVERY_PASS (the context checks its chunks straight away, merged_check 3);
* the structure list under forced Miller-loop shapes (BLS_DEBUG_MLF_PL 1, 2, 4, 3, with and
  without BLS_DEBUG_NO_UNITS) on the aggregated path: f shared between a lane's items or
  not when the failed chunks' requests run their own loops again;
* the knob variants, each in a fresh child process whose environment is set before the
  library loads: $BLS_GROUP_EQ = 0 / 2, group sums on every test / never, the one-lane
  chunk check (its value is not kept), group tests off / from 16 requests.

A pass with a non-batchable request runs no merged check (bls/plan.hpp plan_pass:
merged_eligible), so merged_check == 2 / 3 is asserted on the messages without one, and
the whole list, the two non-batchable requests included (they come first in the
individually verified list and shift every later index), runs with merged_check == 0.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import _recovery as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def ctx(golden):
    """Own context with the 100 interop keys (KAT-2) at table indices 0..99."""
    from lodestar_amd.native import GpuContext

    c = GpuContext(0)
    pks = b"".join(bytes.fromhex(h) for h in golden["kat2_interop_pubkeys"])
    assert (c.load_pubkeys(pks, 48) == 0).all()
    yield c
    c.close()


@pytest.fixture(scope="module", params=["pset", "sigagg"])
def verify_path(request, ctx):
    """Both per-set paths, whatever the call size would pick, the merged check on every pass
    (as in test_gpu_parity.py)."""
    from lodestar_amd._abi import DEBUG_MERGED_EVERY_PASS, DEBUG_SIGAGG_OFF, DEBUG_SIGAGG_ON

    ctx.base_debug_flags = (DEBUG_SIGAGG_ON if request.param == "sigagg" else DEBUG_SIGAGG_OFF) | \
        DEBUG_MERGED_EVERY_PASS
    ctx.set_debug_flags(0)
    yield request.param
    ctx.base_debug_flags = 0
    ctx.set_debug_flags(0)


def _signer(gpu):
    from lodestar_amd import workloads as W

    sks = W.interop_sks(R.N_KEYS)
    return lambda keys, roots: W._sign_all(gpu, [sks[k] for k in keys], roots)


@pytest.fixture(scope="module")
def cases(ctx, oracle):
    """Both lists, packed once with their signatures, and what they must come back as;
    'batchable': the sweep without its non-batchable requests."""
    from lodestar_amd.native import pack_requests

    out = {}
    for name, msgs in (("sweep", R.sweep()), ("structure", R.structure())):
        pbs = [pack_requests(reqs) for reqs in R.materialize(msgs, _signer(ctx), name.encode())]
        exp = R.expectations(oracle, msgs)
        out[name] = (msgs, pbs, exp)
    msgs, pbs, exp = out["sweep"]
    keep = [i for i, m in enumerate(msgs) if all(b for b, _ in m["reqs"])]
    out["batchable"] = ([msgs[i] for i in keep], [pbs[i] for i in keep], [exp[i] for i in keep])
    return out


def _compare(msgs, exp, variant, verdicts, retries, ok, counts, where):
    """verdicts per message, then the summed worker counters, then the round counters"""
    for msg, e, v in zip(msgs, exp, verdicts):
        assert [int(x) for x in v] == e["verdicts"], "%s: verdicts of %s" % (where, R.describe(msg))
    want_retries, want_ok, want_counts = R.totals(exp, variant)
    assert (retries, ok) == (want_retries, want_ok), "%s: worker counters (batch_retries, batch_sigs_success)" % where
    assert list(counts) == want_counts, "%s: round counters, model '%s'%s" % (where, variant, _blame(msgs, exp, variant))


def _blame(msgs, exp, variant):
    """the families' shares of the expected counters, to place a difference"""
    fam = {}
    for m, e in zip(msgs, exp):
        fam[m["family"]] = [a + b for a, b in zip(fam.get(m["family"], [0] * 8), e["counters"][variant])]
    return "; expected by family: " + ", ".join("%s %s" % kv for kv in sorted(fam.items()) if any(kv[1]))


def _run(gpu, case, variant, merged, where, flags=0):
    msgs, pbs, exp = case
    try:
        gpu.set_debug_flags(flags)
        v, st = gpu.verify_many(pbs)
        counts = gpu.group_test_counts()
    finally:
        gpu.set_debug_flags(0)
    _compare(msgs, exp, variant, v, st.batch_retries, st.batch_sigs_success, counts, where)
    assert st.merged_check == merged, "%s: merged_check" % where
    return counts


@pytest.mark.parametrize("which", ["batchable", "structure"])
def test_recovery_default_knobs(ctx, cases, verify_path, which):
    """the merged check fails, the chunks are checked cooperatively (their values kept), and
    every single-invalid chunk is decided in pass A against the chunk check's value; then the
    same call on a context that skips the merged check after a failing pass"""
    from lodestar_amd._abi import DEBUG_MERGED_EVERY_PASS

    where = "%s/%s" % (verify_path, which)
    counts = _run(ctx, cases[which], "eq1_kept", 2, where)
    assert counts[1] > 0 and counts[7] == 0
    base = ctx.base_debug_flags
    try:
        ctx.base_debug_flags = base & ~DEBUG_MERGED_EVERY_PASS
        again = _run(ctx, cases[which], "eq1_kept", 3, where + ", merged check skipped")
    finally:
        ctx.base_debug_flags = base
        ctx.set_debug_flags(0)
    assert again == counts


def test_recovery_with_non_batchable_requests(ctx, cases, verify_path):
    """the whole sweep: its non-batchable requests head the individually verified list"""
    counts = _run(ctx, cases["sweep"], "eq1_kept", 0, "%s/sweep" % verify_path)
    assert counts[1] > 0 and counts[7] == 0


@pytest.mark.parametrize("no_units", [False, True])
@pytest.mark.parametrize("per_lane", [1, 2, 4, 3])
def test_recovery_structure_forced_ml_shapes(ctx, cases, per_lane, no_units):
    """the aggregated path's Miller-loop shapes: at 1 item per lane or per lane pair a set's
    f is its own after the first pass, at 2 and 4 it was shared and the failed chunks' sets
    run their own loops again (plan_own_sets with and without the units' set_unit)"""
    from lodestar_amd._abi import DEBUG_MERGED_EVERY_PASS, DEBUG_MLF_PL, DEBUG_NO_UNITS, DEBUG_SIGAGG_ON

    base = ctx.base_debug_flags
    try:
        ctx.base_debug_flags = DEBUG_SIGAGG_ON | DEBUG_MERGED_EVERY_PASS
        flags = DEBUG_MLF_PL(per_lane) | (DEBUG_NO_UNITS if no_units else 0)
        _run(ctx, cases["structure"], "eq1_kept", 2, "sigagg/structure, pl %d, no_units %s" % (per_lane, no_units), flags)
    finally:
        ctx.base_debug_flags = base
        ctx.set_debug_flags(0)


# ---- the knob variants: one fresh child process each ------------------------------------------

_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.environ["REPO"])
sys.path.insert(0, os.path.join(os.environ["REPO"], "tests"))
import _recovery as R
from lodestar_amd import workloads as W
from lodestar_amd.native import GpuContext, pack_requests
out = {}
with GpuContext(0) as gpu:
    W.load_table([gpu], R.N_KEYS)
    sks = W.interop_sks(R.N_KEYS)
    sign = lambda keys, roots: W._sign_all(gpu, [sks[k] for k in keys], roots)
    for name, msgs in (("sweep", R.sweep()), ("structure", R.structure())):
        pbs = [pack_requests(reqs) for reqs in R.materialize(msgs, sign, name.encode())]
        v, st = gpu.verify_many(pbs)
        out[name] = {"verdicts": [[int(x) for x in w] for w in v], "retries": st.batch_retries,
                     "ok": st.batch_sigs_success, "merged": st.merged_check, "shape": st.pass_shape,
                     "counts": gpu.group_test_counts()}
print(json.dumps(out))
"""

# environment -> the model's variant
KNOBS = {
    "group_eq_0": ({"BLS_GROUP_EQ": "0"}, "eq0_kept"),
    "group_eq_2": ({"BLS_GROUP_EQ": "2"}, "eq2_kept"),
    "group_sums_every_test": ({"BLS_GROUP_SUMS_MIN": "0"}, "eq1_kept"),
    "group_sums_off": ({"BLS_GROUP_SUMS": "0"}, "eq1_kept"),
    "fe_simt": ({"BLS_FE_SIMT_MIN": "1"}, "eq1_lost"),
    "group_test_off": ({"BLS_GROUP_TEST_MIN": "0"}, "gt_off"),
    "group_test_16": ({"BLS_GROUP_TEST_MIN": "16"}, "gt16"),
}


@pytest.fixture(scope="module")
def expected(oracle):
    return {name: (msgs, R.expectations(oracle, msgs)) for name, msgs in (("sweep", R.sweep()), ("structure", R.structure()))}


@pytest.mark.parametrize("case", sorted(KNOBS))
def test_recovery_knob_variants(case, expected):
    knobs, variant = KNOBS[case]
    env = {k: v for k, v in os.environ.items() if not k.startswith("BLS_")}
    env.update(knobs, REPO=str(ROOT))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for name, (msgs, exp) in expected.items():
        g = got[name]
        _compare(msgs, exp, variant, g["verdicts"], g["retries"], g["ok"], g["counts"], "%s/%s" % (case, name))
        # (the sweep holds non-batchable requests: no merged check; the structure list's fails)
        assert g["merged"] == (0 if name == "sweep" else 2), "%s/%s: merged_check" % (case, name)
        assert g["counts"][7] == 0
    if variant in ("eq1_kept", "eq2_kept", "eq0_kept", "eq1_lost"):
        assert (got["sweep"]["counts"][1] > 0) == (variant == "eq1_kept")
