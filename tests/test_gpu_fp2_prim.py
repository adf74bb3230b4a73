"""The out-of-line lazy Fp2 primitives on the GPU (bls/field.hpp fp2_mul_w / fp2_sqr_w), run
exactly as the Miller-loop kernels call them -- the second operand through the lane-private
LDS slot, the result back in registers -- through bls_gpu_field_op_test (kernels/
field_ops.hpp FOP_FP2_MUL_W, FOP_FP2_SQR_W, FOP_FP2_CHAIN_W), word for word against Python
integers.  Inputs: raw Montgomery-form coefficients up to the stated bound (< 2p); outputs
canonical.  What only the device has: one asm statement per row of 14 multiply-adds
(bls/d28_rows.hpp), the calling convention, the slot.  (The same rows in their portable
form, and the bound itself: tests/test_fp2_bound.py.)"""
from __future__ import annotations

import random

import numpy as np
import pytest

from tests import _fieldvec as V
from tests._codec import P

pytestmark = pytest.mark.gpu

R = 1 << 384
R_INV = pow(R, -1, P)
BOUND = 2 * P  # exclusive, every coefficient
# base op ids (csrc/kernels/field_ops.hpp), right after coop_lin's
FP2_MUL_W = V.LIN8 + 1
FP2_SQR_W = FP2_MUL_W + 1
FP2_CHAIN_W = FP2_MUL_W + 2
EDGES = [0, R % P, P - 1, BOUND - 1]  # 0, Montgomery 1, p - 1, the bound - 1


def _mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) * R_INV % P, (a[0] * b[1] + a[1] * b[0]) * R_INV % P)


def _sqr(a):
    return ((a[0] * a[0] - a[1] * a[1]) * R_INV % P, 2 * a[0] * a[1] * R_INV % P)


def _chain(a, b):
    r1 = _mul(a, b)
    r2 = _mul(r1, b)
    r3 = _mul(b, r2)
    return _mul(r3, r1)


def _records():
    rng = random.Random("fp2-prim")
    # every coefficient at every edge (256 records: all at the bound - 1, the largest a1 b1
    # on a0 b0 = 0, ... among them), then 256 random records
    quads = [(a0, a1, b0, b1) for a0 in EDGES for a1 in EDGES for b0 in EDGES for b1 in EDGES]
    quads += [tuple(rng.randrange(BOUND) for _ in range(4)) for _ in range(256)]
    return quads


QUADS = _records()
PAIRS = [(a0, a1) for a0 in EDGES for a1 in EDGES] + [q[:2] for q in QUADS[256:]]


def _pack(vals):
    return np.array([sum((V.limbs(v) for v in rec), []) for rec in vals], dtype=np.uint32)


def _check(out, want, what):
    assert out.shape == (len(want), 24)
    for i, (c0, c1) in enumerate(want):
        got = (V.unlimbs(out[i, :12]), V.unlimbs(out[i, 12:]))
        assert got == (c0, c1), f"{what} record {i}: got ({got[0]:#x}, {got[1]:#x}), want ({c0:#x}, {c1:#x})"


def test_fp2_mul_w(gpu):
    out = gpu.field_op_test(FP2_MUL_W | V.D28, _pack(QUADS))
    _check(out, [_mul(q[:2], q[2:]) for q in QUADS], "fp2_mul_w")


def test_fp2_sqr_w(gpu):
    out = gpu.field_op_test(FP2_SQR_W | V.D28, _pack(PAIRS))
    _check(out, [_sqr(a) for a in PAIRS], "fp2_sqr_w")


def test_partial_second_wavefront(gpu):
    """70 records: one full wavefront and six lanes of a second"""
    recs = QUADS[250:320]  # edge and random records
    assert len(recs) == 70
    out = gpu.field_op_test(FP2_MUL_W | V.D28, _pack(recs))
    _check(out, [_mul(q[:2], q[2:]) for q in recs], "fp2_mul_w (70)")
    out = gpu.field_op_test(FP2_SQR_W | V.D28, _pack([q[:2] for q in recs]))
    _check(out, [_sqr(q[:2]) for q in recs], "fp2_sqr_w (70)")


def test_four_dependent_products_through_one_slot(gpu):
    """a b, (a b) b, b (a b^2), (a b^3)(a b): the slot holds b, b, a b^2, a b in turn -- a
    stale slot or a reordered LDS access changes the result"""
    recs = QUADS[:16] + QUADS[240:330]
    out = gpu.field_op_test(FP2_CHAIN_W | V.D28, _pack(recs))
    _check(out, [_chain(q[:2], q[2:]) for q in recs], "fp2 chain")


def test_shapes(gpu):
    assert gpu.field_op_shape(FP2_MUL_W | V.D28) == (48, 24)
    assert gpu.field_op_shape(FP2_SQR_W | V.D28) == (24, 24)
    assert gpu.field_op_shape(FP2_CHAIN_W | V.D28) == (48, 24)
