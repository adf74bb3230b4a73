"""bls_gpu_verify_same_message without a GPU: the binding and its argument checks, and the
CPU restatement of k_smsum's reduction tree and of the call's host-side plan
(tests/native/smsum_host.cpp: the same bls/smsum.hpp and bls/plan.hpp bodies compiled
for the host), once plain and once under AddressSanitizer + UBSan as a stand-alone
program."""
from __future__ import annotations

import ctypes
import subprocess

import numpy as np

from lodestar_amd._abi import BlsSameMsgBatch, BlsStats, load_library
from lodestar_amd.build import build_smsum_host
from lodestar_amd.native import GpuContext, PackedSameMsg, pack_same_message


def test_binding_exists_and_refuses_bad_arguments_without_a_device():
    lib = load_library()
    assert lib.bls_gpu_verify_same_message.restype is ctypes.c_int
    assert callable(GpuContext.verify_same_message) and callable(GpuContext.verify_same_message_packed)
    b = BlsSameMsgBatch()
    verdicts = np.zeros(4, dtype=np.int32)
    st = BlsStats()
    vp = verdicts.ctypes.data_as(ctypes.c_void_p)
    # no context / no batch: -2 before anything is read
    assert lib.bls_gpu_verify_same_message(None, ctypes.byref(b), vp, ctypes.byref(st)) == -2
    assert lib.bls_gpu_verify_same_message(None, None, vp, None) == -2
    b.n_jobs, b.n_sets = 1, 0  # an empty job, still without a device
    assert lib.bls_gpu_verify_same_message(None, ctypes.byref(b), vp, ctypes.byref(st)) == -2
    assert (verdicts == 0).all()


def test_pack_same_message_layout():
    ps = pack_same_message([(b"\x01" * 32, [5, 6], [b"\x02" * 96, b"\x03" * 96]), (b"\x04" * 32, [7], [b"\x05" * 96])],
                           seed=b"\x09" * 32)
    assert isinstance(ps, PackedSameMsg) and ps.n_jobs == 2 and ps.n_sets == 3
    assert list(ps.job_set_offsets) == [0, 2, 3] and list(ps.pk_indices) == [5, 6, 7]
    assert ps.messages.tobytes() == b"\x01" * 32 + b"\x04" * 32
    assert ps.signatures.tobytes() == b"\x02" * 96 + b"\x03" * 96 + b"\x05" * 96
    empty = pack_same_message([])
    assert empty.n_jobs == 0 and empty.n_sets == 0


def test_python_verifier_dispatch_with_a_stand_in_context():
    """Host side of GpuBlsVerifier.verify_signature_sets_same_message over a stand-in
    context (no GPU): table-index sets form one job of their own kind, jobs queued together
    reach a context in ONE native call, a code other than 1 is False, an int that is no
    uint32 is False without a call, the weight is the set count."""
    import threading

    from lodestar_amd.verifier import GpuBlsVerifier

    gate, entered = threading.Event(), threading.Event()

    class Ctx:
        def __init__(self):
            self.calls = []

        def load_pubkeys(self, b, n):
            return np.zeros(1, np.int32)

        def verify_same_message(self, jobs, seed=None):
            entered.set()
            gate.wait(10)
            self.calls.append([len(j[1]) for j in jobs])
            return [np.array([1 if i % 2 == 0 else -1 for i in j[1]], np.int32) for j in jobs], BlsStats()

        def close(self):
            pass

    sig = b"s" * 96
    with GpuBlsVerifier(n_contexts=1, context_factory=lambda dev, high: Ctx()) as v:
        first = v.verify_signature_sets_same_message_async([(0, sig), (1, sig), (-5, sig), (2, sig)], b"m" * 32)
        # queued while the context is busy with the first call: taken together afterwards
        assert entered.wait(10)
        fa = v.verify_signature_sets_same_message_async([(0, sig)] * 3, b"a" * 32)
        fb = v.verify_signature_sets_same_message_async([(1, sig)] * 2, b"b" * 32)
        gate.set()
        assert first.result(10) == [True, False, False, True]
        assert fa.result(10) == [True] * 3 and fb.result(10) == [False] * 2
        assert v._ctxs[0].calls == [[3], [3, 2]]
        assert v.slot_stats[0] == {"calls": 2, "sets": 8, "weight": 8.0}
        assert v.verify_signature_sets_same_message([(-1, sig)], b"m" * 32) == [False]
        assert v.verify_signature_sets_same_message([], b"m" * 32) == []


def test_addon_and_js_verifier_export_the_call():
    import shutil
    from pathlib import Path

    import pytest

    root = Path(__file__).resolve().parent.parent
    addon = root / "lodestar_amd" / "_native" / "lodestar_bls.node"
    node = shutil.which("node")
    if node is None or not addon.exists():
        pytest.skip("node or the N-API addon is absent")
    code = ("const a = require(process.argv[1]); const m = require(process.argv[2]);"
            "const r = m.packSameMessage([{message: Buffer.alloc(32, 1), indices: [4, 9],"
            " signatures: [Buffer.alloc(96, 2), Buffer.alloc(96, 3)]}, {message: Buffer.alloc(32, 5), indices: [7],"
            " signatures: [Buffer.alloc(96, 6)]}]);"
            "console.log(JSON.stringify([typeof a.verifySameMessage,"
            " typeof m.GpuBlsVerifier.prototype.verifySignatureSetsSameMessage, Array.from(r.jobSetOffsets),"
            " Array.from(r.pkIndices), r.messages.length, r.signatures[96], r.signatures[192]]))")
    out = subprocess.run([node, "-e", code, str(addon), str(root / "integration" / "js" / "gpuBlsVerifier.js")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    import json

    assert json.loads(out.stdout) == ["function", "function", [0, 2, 3], [4, 9, 7], 64, 3, 6]


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 50, out.stdout[-500:]


def test_smsum_tree_matches_left_to_right_sum():
    """job sizes 1, 2, 63, 64, 65 and 129 with some sets not live (and a job whose live sets
    cancel): the 64-lane strided sums and the six-step tree equal the plain sum in affine
    form, smsum_finish writes the unit and the virtual set, the plan maps jobs to chunks"""
    _run(build_smsum_host(verbose=False))


def test_smsum_and_planner_under_sanitizers(tmp_path):
    """the same stand-alone program (the host-side planner and the tree) compiled with
    -fsanitize=address,undefined: any report makes it exit non-zero"""
    exe = build_smsum_host(verbose=False, out=tmp_path / "smsum_host_san",
                           extra=["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _run(exe)
