"""The device self-test's vectors and references (tests/_fieldvec.py) checked on the CPU:
the same records through the CPU build of the same headers (tests/native/hostsim.cpp)
must pass the very checks the GPU output gets, so a wrong reference or a malformed
record shows here, before any GPU run.  (The device-only code -- the inline-asm carry
chains and multiply-adds, the 32-bit column product, the interpreter's accumulator --
is what tests/test_gpu_field_ops.py then runs on the GPU.)"""
from __future__ import annotations

import ctypes

import pytest

from tests import _fieldvec as V
from tests._codec import P, b48, f2b, fp

SETS = V.sets()


def test_case_list_matches_sets():
    assert tuple(SETS) == V.SET_NAMES
    assert {nm for nm, s in SETS.items() if s.d28_only} == V.D28_ONLY
    assert V.CASES == [(nm, fl) for nm, s in SETS.items() for fl in s.flavours]


def test_records_match_the_library_shapes():
    """every record packs to the op's input size in the C table; launches stay under
    1,000 lanes with a partial last wavefront; unknown ops are refused"""
    from lodestar_amd._abi import load_library

    lib = load_library()
    iw, ow = ctypes.c_uint32(), ctypes.c_uint32()
    for s in SETS.values():
        assert len(s.records) % 64 != 0 and len(s.records) < 1000, s.name
        for fl in s.flavours:
            assert lib.bls_gpu_field_op_shape(s.op | fl, ctypes.byref(iw), ctypes.byref(ow)) == 0, s.name
            for rec in s.records:
                w = s.pack(rec)
                assert len(w) == iw.value and all(0 <= x < 1 << 32 for x in w), s.name
        if s.d28_only:
            assert lib.bls_gpu_field_op_shape(s.op, ctypes.byref(iw), ctypes.byref(ow)) == -2, s.name
    assert lib.bls_gpu_field_op_shape(V.PREDS + 1, ctypes.byref(iw), ctypes.byref(ow)) == -2
    assert lib.bls_gpu_field_op_shape(0x200, ctypes.byref(iw), ctypes.byref(ow)) == -2


def test_lin8_vectors_cover_the_issue_edges():
    recs = SETS["coop_lin"].records
    top = 3 * P - 1
    assert ((top,) * 8, (V.CMAX,) * 8, 8, 0) in recs and ((top,) * 8, (-V.CMAX,) * 8, 8, 0) in recs
    assert ((top,) * 8, (V.CMAX, -V.CMAX) * 4, 8, 0) in recs
    assert {r[2] for r in recs} == set(range(9))
    assert {r[3] for r in recs if r[2] == 1 and r[1][0] == 1} == {0, 1}  # one +1 term: both paths
    totals = [V.lin8_total(r) for r in recs]
    assert any(t == 0 and r[2] > 0 for t, r in zip(totals, recs))
    assert any(t != 0 and t % P == 0 and t > 0 for t in totals) and any(t % P == 0 and t < 0 for t in totals)
    assert 3 * 8 * V.CMAX == 786408 <= 1 << 20


def test_lin8_vectors_against_the_accumulator_model():
    """acc_reduce modelled in Python (the quotient estimate in the device's double
    arithmetic): every record lands in [0, 3p) with the right residue, and the set holds
    records on which the quotient estimate is not below the true quotient, so that "q"
    in place of "q - 1" wraps below zero there."""
    wrapped = 0
    for rec in SETS["coop_lin"].records:
        t = V.lin8_total(rec)
        r = V.acc_reduce_model(t)
        assert 0 <= r < 3 * P and r % P == t % P
        wrapped += V.acc_reduce_model(t, q_minus=0) < 0
    assert wrapped >= 10


def _le(v):
    return v.to_bytes(48, "little")


def _words(raw: bytes):
    return [int.from_bytes(raw[4 * k: 4 * k + 4], "little") for k in range(len(raw) // 4)]


def _run_host(hostsim, name, rec):
    """output words of set `name`'s record through the hostsim entry point of the same function"""
    o = ctypes.create_string_buffer(576)
    if name in ("fp_add", "fp_sub"):
        getattr(hostsim, "hs_" + name)(b48(rec[0]), b48(rec[1]), o)
        return V.limbs(fp(o.raw[:48]))
    if name == "fp_half":
        hostsim.hs_fp_half(b48(rec[0]), o)
        return V.limbs(fp(o.raw[:48]))
    if name in ("fp_mul", "fp_mul_lazy", "fp_sqr", "fp_sqr_d28_lazy"):
        sqr = len(rec) == 1
        hostsim.hs_fp_mul_d28_raw(_le(rec[0]), _le(rec[0] if sqr else rec[1]), o, int(sqr))
        r = int.from_bytes(o.raw[:48], "little")
        if name in ("fp_mul", "fp_sqr"):  # the device's fp_mul / fp_sqr: fp_reduce_once of the lazy product
            assert r < 2 * P
            r = r - P if r >= P else r
        return V.limbs(r)
    if name in ("fp2_mul_d28", "fp2_mul_s"):
        fn = hostsim.hs_fp2_mul_d28_raw if name == "fp2_mul_d28" else hostsim.hs_fp2_mul_s_raw
        fn(_le(rec[0]) + _le(rec[1]), _le(rec[2]) + _le(rec[3]), o)
        return _words(o.raw[:96])
    if name == "fp2_sqr_d28":
        hostsim.hs_fp2_sqr_d28_raw(_le(rec[0]) + _le(rec[1]), o)
        return _words(o.raw[:96])
    if name in ("lz_mul_w", "lz_sqr_w"):
        out = (ctypes.c_int32 * 14)()
        x, y = (ctypes.c_int32 * 14)(*rec[0]), (ctypes.c_int32 * 14)(*rec[1])
        hostsim.hs_lz_mul_raw(x, x if name == "lz_sqr_w" else y, out, int(name == "lz_sqr_w"))
        return [d & 0xFFFFFFFF for d in out]
    if name == "lz_fp_ops":
        hostsim.hs_lz_fp_ops(b48(rec[0]), b48(rec[1]), o)
        return [w for k in range(10) for w in V.limbs(V.mont(fp(o.raw[48 * k: 48 * k + 48])))]
    if name == "lz_fp2_ops":
        hostsim.hs_lz_fp2_ops(f2b(rec[0]), f2b(rec[1]), o)
        return [w for k in range(12) for w in V.limbs(V.mont(fp(o.raw[48 * k: 48 * k + 48])))]
    if name == "fp_inv_gcd":
        hostsim.hs_fp_inv_gcd(b48(rec[0]), o)
        return V.limbs(V.mont(fp(o.raw[:48])))
    if name == "fp_sqrt":
        ok = hostsim.hs_fp_sqrt(b48(rec[0]), o)
        return [int(ok)] + V.limbs(V.mont(fp(o.raw[:48])))
    if name == "fp2_sqrt":
        ok = hostsim.hs_fp2_sqrt(f2b(rec), o)
        return [int(ok)] + V.limbs(V.mont(fp(o.raw[:48]))) + V.limbs(V.mont(fp(o.raw[48:96])))
    if name == "preds":
        return [hostsim.hs_preds_raw(_le(rec[0]) + _le(rec[1])) & 0xFFFFFFFF]
    raise KeyError(name)


HOST_SETS = ("fp_add", "fp_sub", "fp_half", "fp_mul", "fp_sqr", "fp_mul_lazy", "fp_sqr_d28_lazy", "fp2_mul_d28",
             "fp2_sqr_d28", "fp2_mul_s", "lz_mul_w", "lz_sqr_w", "lz_fp_ops", "lz_fp2_ops", "fp_inv_gcd", "fp_sqrt",
             "fp2_sqrt", "preds")


@pytest.mark.parametrize("name", HOST_SETS)
def test_vectors_against_hostsim(hostsim, name):
    s = SETS[name]
    for i, rec in enumerate(s.records):
        err = s.check(rec, _run_host(hostsim, name, rec))
        assert err is None, f"{name} record {i}: {err}"


@pytest.mark.parametrize("name", [nm for nm in V.SET_NAMES if nm not in HOST_SETS])
def test_checks_accept_the_exact_result(name):
    """the sets without a hostsim counterpart: the check accepts the exact answer computed
    here with Python integers, and refuses it with one bit flipped"""
    s = SETS[name]
    exact = {
        "fp_neg": lambda a: -a % P, "fp_dbl": lambda a: 2 * a % P, "fp_add_nr": lambda a, b: a + b,
        "fp_sub_nr": lambda a, b: a + P - b, "fp_reduce_once": lambda a: a % P,
        "fp_reduce_2p": lambda a: a - 2 * P if a >= 2 * P else a, "fp_canon3": lambda a: a % P,
    }
    for rec in s.records[:80]:
        if name in exact:
            out = V.limbs(exact[name](*rec))
        elif name in ("fp2_mul", "fp2_sqr"):
            ref = V._fp2_mul_ref(*rec) if name == "fp2_mul" else V._fp2_sqr_ref(*rec)
            out = V.limbs(ref[0] % P) + V.limbs(ref[1] % P)
        elif name == "fp_inv":
            out = V.limbs(V.mont(pow(rec[0], -1, P)))
        elif name == "fp2_inv":
            ni = pow(rec[0] * rec[0] + rec[1] * rec[1], -1, P)
            out = V.limbs(V.mont(rec[0] * ni % P)) + V.limbs(V.mont(-rec[1] * ni % P))
        else:
            assert name == "coop_lin"
            out = V.limbs(rec[0][0] if rec[3] else V.acc_reduce_model(V.lin8_total(rec)))
        assert s.check(rec, out) is None, name
        bad = list(out)
        bad[5] ^= 1 << 7
        assert s.check(rec, bad) is not None, name
