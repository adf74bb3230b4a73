"""The Fp6 / Fp12 tower of the SIMT verify path, function by function, on the GPU against the
oracle's schoolbook Fp12 on Python integers (bls_gpu_tower_op_test; vectors and references:
tests/_towervec.py, proved on the CPU by tests/test_towervec_cpu.py).

The verify path reaches this layer only through COP_MILLER and whole verdicts -- values
compared after a final exponentiation, which kills any wrong factor in a proper subfield, on
curve points, whose coefficients never sit at an extreme -- and tests/test_hostsim.py
compiles the host's 64-bit product, not the device's.  Here each function runs alone on raw
words, in the translation unit production compiles it in (the 32-bit column product of the
exact path, the 28-bit digits of k_fin_simt.hip, the 28-bit digits over the out-of-line Fp2
primitive of k_mlq.hip, the inlined copies that exist only in those two files), at the raw
coefficient extremes where the Karatsuba pre-additions that are left unreduced reach their
largest operands: a wrong value names its function, record and coefficient.

Every comparison is exact, and every output Fp must be canonical (< p): all these functions
end in fp_add / fp_sub / fp_neg of canonical values or in a product documented "canonical
out" (bls/field.hpp).  Every test is one launch of at most a few hundred lanes."""
from __future__ import annotations

import numpy as np
import pytest

from tests import _towervec as V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,flavour", V.CASES, ids=V.CASE_IDS)
def test_tower_op(gpu, name, flavour):
    """one launch: every record of the op through the production function.  The pair ops run
    an odd record count, so the last pair shares its wavefront with idle lanes."""
    t = V.OPS[name]
    records = t.records
    if t.out == "pair" and len(records) % 2 == 0:
        records = records[:-1]
    out = gpu.tower_op_test(t.op | flavour, np.array([V.pack(r.operands) for r in records], dtype=np.uint32))
    assert out.shape[0] == len(records)
    for i, rec in enumerate(records):
        err = t.check(rec, [int(w) for w in out[i]])
        assert err is None, V.failure(t, flavour, i, rec, err)


def test_line_buffer(gpu):
    """k_mlq<1> alone over six items (Jacobian z random and z = 1): each item's 68 lines as
    store_line wrote them, against the restated steps over the oracle's Fp2"""
    items = V.line_items()
    out = gpu.tower_op_test(V.MLQ_LINES | V.D28, np.array([V.pack_line_item(it) for it in items], dtype=np.uint32))
    for i, it in enumerate(items):
        err = V.check_lines(it, [int(w) for w in out[i]])
        assert err is None, f"lines in {V.TU_MLQ} (k_mlq), item {i} [z {'= 1' if it[1] == 1 else 'random'}]: {err}"


def test_tower_op_refusals(gpu):
    """an op in a flavour it does not exist in, and an unknown op, return the error, launch
    nothing and leave out_words untouched; records of the wrong shape are refused"""
    from lodestar_amd.native import NativeError

    wrong = [t.op | fl for t in V.OPS.values() for fl in (0, V.D28) if fl not in t.flavours]
    wrong += [V.MLQ_LINES, V.N_OPS, V.N_OPS | V.D28, 0x200, 0xFFFFFFFF]
    assert len(wrong) == 18 + 5  # every op but fp6_mul lacks one flavour
    for op in wrong:
        with pytest.raises(NativeError):
            gpu.tower_op_shape(op)
        rec = np.full((2, 288), 0x5A5A5A5A, dtype=np.uint32)
        out = np.full((2, 288), 0xC3C3C3C3, dtype=np.uint32)
        rc = gpu.lib.bls_gpu_tower_op_test(gpu._h, op, rec.ctypes.data, 2, out.ctypes.data)  # the C entry point itself
        assert rc == -2, hex(op)
        assert (out == 0xC3C3C3C3).all(), hex(op)
    assert gpu.tower_op_shape(V.FP6_MUL) == gpu.tower_op_shape(V.FP6_MUL | V.D28) == (144, 72)
    assert gpu.tower_op_shape(V.FP6_MUL_01) == (120, 72) and gpu.tower_op_shape(V.FP6_MUL_1) == (96, 72)
    assert gpu.tower_op_shape(V.FP12_MUL_LINE) == (216, 144) and gpu.tower_op_shape(V.MLQ_MUL_LINE2 | V.D28) == (288, 144)
    assert gpu.tower_op_shape(V.MLQ_SQR12_PAIR | V.D28) == (144, 288)
    assert gpu.tower_op_shape(V.MLQ_MUL_LINE12_PAIR | V.D28) == (216, 288)
    assert gpu.tower_op_shape(V.MLQ_LINES | V.D28) == (84, 72 * V.LINE_EVENTS)
    with pytest.raises(ValueError):
        gpu.tower_op_test(V.FP12_SQR, np.zeros((3, 145), dtype=np.uint32))
    with pytest.raises(NativeError):
        gpu.tower_op_test(V.MLQ_LINES | V.D28, np.zeros((65, 84), dtype=np.uint32))  # more than 64 items
    assert gpu.tower_op_test(V.FP12_SQR, np.zeros((0, 144), dtype=np.uint32)).shape == (0, 144)
