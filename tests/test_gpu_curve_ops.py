"""The curve-level code of the SIMT verify path, function by function, on the GPU against
the oracle's Python integers (bls_gpu_curve_op_test; vectors and references:
tests/_curvevec.py, proved on the CPU by tests/test_curvevec_cpu.py).

The verify path reaches k_pre's hash_to_field and fast SSWU map, k_chain's role 0 (the
Jacobian isogeny, the regrouped cofactor clearing, the affine conversion) and the exact
path's affine forms only through one verdict bit per request, and only on inputs that come
out of SHA-256.  Here each function runs alone, in the translation-unit flavour production
compiles it in, on directed inputs: a wrong value names its kernel, record and coordinate.

Bounds asserted on the raw output words, per op (bls/field.hpp): every Fp of every op is
canonical (< p) -- FROM_BE64 and H2F end in fp_add; SSWU, SSWU_FAST, ISO_AFF,
CLEAR_COFACTOR end in fp2_mul / fp2_neg / fp_neg of canonical values (fp_mul without LAZY
is canonical in both products); ISO_JAC and CHAIN_H end in the out-of-line Fp2 product
("canonical out"), jac_infinity's constants, or fp2_neg; MILLER's f is fp12_conj of sums
and differences (fp_add / fp_sub / fp_neg reduce) of such products.  Every test is one or
two calls of at most a few hundred lanes."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import bls_oracle as O
from tests import _curvevec as V

pytestmark = pytest.mark.gpu


def _run(gpu, s, flavour, records):
    recs = np.array([s.pack(r) for r in records], dtype=np.uint32)
    out = gpu.curve_op_test(s.op | flavour, recs)
    assert out.shape[0] == len(records)
    return out


@pytest.mark.parametrize("name,flavour", V.CASES, ids=V.CASE_IDS)
def test_curve_op(gpu, name, flavour):
    """one launch: every record of the op's vector set through the production function"""
    s = V.SETS[name]
    records = s.records()
    out = _run(gpu, s, flavour, records)
    for i, rec in enumerate(records):
        err = s.check(rec, [int(w) for w in out[i]])
        assert err is None, V.failure(s, flavour, i, rec, err)


def test_sswu_fast_refuses_exactly_the_exceptional_inputs(gpu):
    """ok = 0 on u = 0 and on the u whose g(x1) lies in Fp (both signs), ok = 1 elsewhere"""
    s = V.SETS["sswu_fast"]
    us = s.records()
    out = _run(gpu, s, V.D28, us)
    refused = {u for u, o in zip(us, out) if int(o[0]) == 0}
    c1 = set(V.c1_zero_pick())
    assert refused == {(0, 0)} | c1 | {O.f2_neg(u) for u in c1}
    assert all(int(o[0]) in (0, 1) for o in out)


def test_chain_h_is_hash_to_g2_bit_for_bit(gpu):
    """64 messages through the device's own H2F and SSWU_FAST, their raw words fed forward
    into k_chain's role 0 unchanged (two launches before it): HQ is the oracle's
    hash_to_g2(message), the H of the verify path"""
    msgs = V.chain_messages()
    u = gpu.curve_op_test(V.H2F | V.D28, np.array([V.pack_msg(m) for m in msgs], dtype=np.uint32))
    q = gpu.curve_op_test(V.SSWU_FAST | V.D28, u.reshape(2 * len(msgs), 24))
    assert all(int(r[0]) == 1 for r in q), "map_to_curve_sswu_fast refused a hashed u"
    out = gpu.curve_op_test(V.CHAIN_H | V.D28, np.ascontiguousarray(q[:, 1:]).reshape(len(msgs), 96))
    s = V.SETS["chain_h"]
    for i, m in enumerate(msgs):
        err = V.check_chain_h(O.hash_to_g2(m), [int(w) for w in out[i]])
        assert err is None, f"chain_h in {s.where(V.D28)}, message {i} [{m.hex()}]: {err}"


@pytest.mark.parametrize("per_lane", V.PER_LANES, ids=["1", "2", "4", "pair"])
def test_miller_loops_through_the_launchers(gpu, per_lane):
    """launch_k_mlqf over 27 items in domains of 1..5 (k_mlq, then k_mlf at 1, 2, 4 items per
    lane or k_mlf2): per domain FE(prod f_i), computed by the oracle from the device's f,
    equals FE(prod oracle.miller_loop(P_i, Q_i)), both with the exponent 3 (p^12 - 1) / r; an
    item that shared another's f holds exactly 1"""
    recs = np.array([V.pack_miller(it, per_lane) for it in V.miller_items()], dtype=np.uint32)
    out = gpu.curve_op_test(V.MILLER | V.D28, recs)
    err = V.check_miller(per_lane, [[int(w) for w in row] for row in out],
                         f"miller in k_mlq + {'k_mlf2' if per_lane == V.MLF_PAIR else f'k_mlf ({per_lane} per lane)'}")
    assert err is None, err


def test_miller_is_bilinear(gpu):
    """f(aP, Q) and f(P, aQ) agree after the final exponentiation"""
    recs = np.array([V.pack_miller(it, 1) for it in V.bilinear_items()], dtype=np.uint32)
    out = gpu.curve_op_test(V.MILLER | V.D28, recs)
    fe = []
    for row in out:
        vals, err = V.fps_out([int(w) for w in row], V.F12_NAMES)
        assert err is None, err
        fe.append(O.final_exponentiation(V.f12_unpack(vals), 3))
    assert fe[0] == fe[1] and not O.f12_is_one(fe[0])


def test_final_exponentiation_both_forms(gpu):
    """FE(F) == 1 by k_chunk_simt (fe_is_one) and by the cooperative chunk kernel, one chunk
    per task, against the oracle's final_exponentiation(F, 3); the r-th powers among the
    tasks are the ones on which a wrong hard-part exponent turns a 1 into a 0"""
    tasks = V.fe_tasks()
    out = gpu.curve_op_test(V.FE | V.D28, np.array([V.f12_pack(f) for _nm, f in tasks], dtype=np.uint32))
    for k, (nm, _f) in enumerate(tasks):
        want = int(V.ref_fe_is_one(k))
        assert int(out[k][0]) == want, f"fe in k_fin_simt (k_chunk_simt), task {k} [{nm}]: chunk_ok = {int(out[k][0])}, want {want}"
        assert int(out[k][1]) == want, f"fe in k_fin (k_chunk_coop), task {k} [{nm}]: chunk_ok = {int(out[k][1])}, want {want}"


def test_curve_op_refusals(gpu):
    """unknown ops, ops in a flavour they do not exist in, and records of the wrong shape"""
    from lodestar_amd.native import NativeError

    for s in V.SETS.values():
        for fl in (0, V.D28):
            if fl not in s.flavours:
                with pytest.raises(NativeError):
                    gpu.curve_op_shape(s.op | fl)
                with pytest.raises(NativeError):
                    gpu.curve_op_test(s.op | fl, np.zeros((1, 48), dtype=np.uint32))
    for op in (V.MILLER, V.FE, V.FE + 1, (V.FE + 1) | V.D28, 0x200, 0xFFFFFFFF):
        with pytest.raises(NativeError):
            gpu.curve_op_shape(op)
    assert gpu.curve_op_shape(V.SSWU_FAST | V.D28) == (24, 49) and gpu.curve_op_shape(V.CHAIN_H | V.D28) == (96, 49)
    assert gpu.curve_op_shape(V.ISO_JAC | V.D28) == (48, 72) and gpu.curve_op_shape(V.FROM_BE64) == (16, 12)
    with pytest.raises(ValueError):
        gpu.curve_op_test(V.SSWU, np.zeros((3, 25), dtype=np.uint32))
    with pytest.raises(ValueError):
        gpu.curve_op_test(V.H2F | V.D28, np.zeros(8, dtype=np.uint32))
    rc = gpu.lib.bls_gpu_curve_op_test(gpu._h, V.SSWU | V.D28, None, 1, None)  # the C entry point itself
    assert rc == -2
    assert gpu.curve_op_test(V.H2F, np.zeros((0, 8), dtype=np.uint32)).shape == (0, 48)
    assert gpu.curve_op_shape(V.MILLER | V.D28) == (86, 144) and gpu.curve_op_shape(V.FE | V.D28) == (144, 2)
    bad = np.array([V.pack_miller(V.bilinear_items()[0], 5)], dtype=np.uint32)  # no such items-per-lane
    with pytest.raises(NativeError):
        gpu.curve_op_test(V.MILLER | V.D28, bad)
