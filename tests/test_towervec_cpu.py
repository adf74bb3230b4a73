"""The tower-op self-test's vectors and references (tests/_towervec.py) checked on the CPU:
the references agree with independent statements of the same maps (f12_pow by p and p^2 for
the Frobenius maps, O.miller_loop for the restated line steps), every edge record really has
the raw pattern it is named for, the records named for it reach the largest operand of each
unreduced Karatsuba sum, and the same records through the CPU build of the same headers
(tests/native/hostsim.cpp) pass the very checks the GPU output gets -- so a wrong reference
or a malformed record shows here, before any GPU run.  (What the device compiles differently
-- the 32-bit column product, the 28-bit digits, the out-of-line Fp2 primitive, the inlined
copies in k_mlq.hip and k_fin_simt.hip -- is what tests/test_gpu_tower_ops.py then runs.)"""
from __future__ import annotations

import ctypes
import random

import pytest

from oracle import bls_oracle as O
from tests import _curvevec as C
from tests import _towervec as V
from tests._codec import bf2, f2b

P = O.P


def test_case_list_and_library_shapes():
    """every record packs to the op's input size in the C table; an op is refused in the
    flavour it does not exist in, and past the table"""
    from lodestar_amd._abi import load_library

    lib = load_library()
    iw, ow = ctypes.c_uint32(), ctypes.c_uint32()
    assert len(V.OPS) == V.N_OPS - 1 and sorted(t.op for t in V.OPS.values()) == list(range(V.N_OPS - 1))
    assert len(V.CASES) == 20
    for t in V.OPS.values():
        n_out = {"f6": 72, "f12": 144, "pair": 288}[t.out]
        assert 10 <= len(t.records) <= 110, (t.name, len(t.records))
        for fl in (0, V.D28):
            rc = lib.bls_gpu_tower_op_shape(t.op | fl, ctypes.byref(iw), ctypes.byref(ow))
            assert rc == (0 if fl in t.flavours else -2), (t.name, fl)
            if rc == 0:
                assert ow.value == n_out
                for rec in t.records:
                    w = V.pack(rec.operands)
                    assert len(w) == iw.value and all(0 <= x < 1 << 32 for x in w), t.name
    assert lib.bls_gpu_tower_op_shape(V.MLQ_LINES, ctypes.byref(iw), ctypes.byref(ow)) == -2
    assert lib.bls_gpu_tower_op_shape(V.MLQ_LINES | V.D28, ctypes.byref(iw), ctypes.byref(ow)) == 0
    assert (iw.value, ow.value) == (84, 72 * V.LINE_EVENTS) and len(V.pack_line_item(V.line_items()[0])) == 84
    for op in (V.N_OPS, V.N_OPS | V.D28, 0x200):
        assert lib.bls_gpu_tower_op_shape(op, ctypes.byref(iw), ctypes.byref(ow)) == -2
    assert 2 <= len(V.line_items()) <= 8


def test_edge_records_have_their_raw_patterns():
    """every record named for a raw pattern has it, on the words as they are packed; every raw
    coefficient of every record is in [0, p); each operand of each op meets every pattern"""
    for t in V.OPS.values():
        if t.make.__name__ == "cyclotomic_records" or t.name in ("cyc_sqr", "exp_x_m"):
            continue
        seen = {j: set() for j in range(len(t.kinds))}
        for rec in t.records:
            words = V.pack(rec.operands)
            at = 0
            for j, kind in enumerate(t.kinds):
                n = 2 * V.KIND_N2[kind]
                raw = C.raw_fps(words, n, at=at)
                at += 12 * n
                assert raw == list(rec.operands[j]) and all(0 <= v < P for v in raw), (t.name, rec.label)
                for jj, nm in rec.tags:
                    if jj == j:
                        assert V.has_pattern(kind, nm, raw), (t.name, rec.label)
                        seen[j].add(nm)
        for j, kind in enumerate(t.kinds):
            want = {nm for nm, _raw in V.edge_operands(kind, random.Random(1))}
            if t.ref is None:
                want.discard("zero")  # 0 has no inverse
            assert seen[j] == want, (t.name, j, want - seen[j])
        assert sum(r.label.startswith("random ") for r in t.records) == V.N_RANDOM, t.name
    labels = [r.label for r in V.OPS["fp12_mul"].records]
    assert "b = conj(a), a random" in labels and "b = conj(a), a all p-1" in labels
    rec = next(r for r in V.OPS["mul12m_conj"].records if r.label == "b = conj(a), a random")
    a, b = (V.element("f12", raw) for raw in rec.operands)
    assert b == O.f12_conj(a)
    labels = [r.label for r in V.OPS["fp12_mul_line2"].records]
    assert "both lines p-1, f random" in labels and "the two lines equal (random), f random" in labels
    assert "every operand p-1" in labels and "both lines neg, f random" in labels
    for t in V.OPS.values():
        if t.ref is None:
            assert all(any(r.operands[0]) for r in t.records)
    for nm in ("only c0.c0", "only Fp2 0", "only c0", "only c1"):  # a in Fp, in Fp2, in Fp6, with c0 = 0
        assert any(r.tags == ((0, nm),) for r in V.OPS["fp12_inv"].records), nm


def _rec(name, label):
    return next(r for r in V.OPS[name].records if r.label == label)


def test_which_record_reaches_which_sites_largest_operand():
    """Every fp2_add_nr result that enters fp2_mul_s in fp6_mul, fp6_mul_01 and fp12_mul_line2 is
    the sum of two canonical coefficients, so at most 2p - 2 (bls/field.hpp, beside each site).
    Which records reach it, on the raw integers:
      * the all-p-1 record of fp6_mul and of fp6_mul_01: every site of the function itself;
      * the all-p-1 record of fp12_mul / mul12m: the sites of t0 = a.c0 b.c0 and t1 = a.c1 b.c1,
        but NOT those of (a.c0 + a.c1)(b.c0 + b.c1), whose operands are the reduced sums p - 2
        (2p - 4 there); the all-(p-1)/2 record reaches them (its reduced sums are p - 1);
        mul12m<true> adds -m.c1, so there it is the record a = (p-1)/2, m = ((p-1)/2, (p+1)/2);
      * the all-p-1 record of fp12_mul_line / mul_line12: the first fp6_mul_01 (aa), not the
        second (2p - 4 and 2p - 3); the record f = (p-1)/2, l0 = p - 1, l2 = l3 = (p-1)/2 does;
      * the all-p-1 lines of fp12_mul_line2: the three products of the lines' sums."""
    top = 2 * P - 2
    p1_6 = [(P - 1, P - 1)] * 3
    assert set(V.sites_fp6_mul(p1_6, p1_6).values()) == {top}
    r = _rec("fp6_mul", "every operand p-1")
    assert set(V.sites_fp6_mul(V._f2s(r.operands[0]), V._f2s(r.operands[1])).values()) == {top}
    r = _rec("fp6_mul_01", "every operand p-1")
    d = V._f2s(r.operands[1])
    assert set(V.sites_fp6_mul_01(V._f2s(r.operands[0]), d[0], d[1]).values()) == {top}
    for name in ("fp12_mul", "mul12m_conj"):
        conj = name == "mul12m_conj"
        s = V.sites_fp12_mul(*_rec(name, "every operand p-1").operands, conj=conj)
        outer = {k: v for k, v in s.items() if k.startswith("t")}
        inner = {k: v for k, v in s.items() if not k.startswith("t")}
        assert len(outer) == 6 and set(outer.values()) == {top}
        assert len(inner) == 3 and set(inner.values()) == {top - 2}
    s = V.sites_fp12_mul(*_rec("fp12_mul", "every operand half-").operands)
    assert all(v == top for k, v in s.items() if not k.startswith("t"))
    s = V.sites_fp12_mul(*_rec("mul12m_conj", "inner max: a half-, m = (half-, half+)").operands, conj=True)
    assert all(v == top for k, v in s.items() if not k.startswith("t"))
    s = V.sites_mul_line(*_rec("fp12_mul_line", "every operand p-1").operands)
    assert s == {"aa: fp6_mul_01 c1": top, "(f.c0 + f.c1): fp6_mul_01 c1": top - 1}
    assert V.LINE_INNER_MAX in V.OPS["mul_line12"].records and V.LINE_INNER_MAX in V.OPS["mul_line12_pair"].records
    s = V.sites_mul_line(*V.LINE_INNER_MAX.operands)
    assert s["(f.c0 + f.c1): fp6_mul_01 c1"] == top
    f, l = V._f2s(V.LINE_INNER_MAX.operands[0]), V._f2s(V.LINE_INNER_MAX.operands[1])
    assert V._add_nr(V._add(f[0], f[3]), V._add(f[1], f[4])) == (top, top) and V._add_nr(l[0], V._add(l[1], l[2])) == (top, top)
    r = _rec("fp12_mul_line2", "every operand p-1")
    assert set(V.sites_line2_lines(r.operands[1], r.operands[2]).values()) == {top}
    # the two ends of the Fp2 product's a0 b0 - a1 b1 at that bound: sums (2p-2, 0) and (0, 2p-2)
    for nm, want in (("c0s p-1", (top, 0)), ("c1s p-1", (0, top))):
        r = _rec("fp6_mul", f"every operand {nm}")
        a = V._f2s(r.operands[0])
        assert V._add_nr(a[1], a[2]) == V._add_nr(a[0], a[1]) == want
        r = _rec("fp12_mul_line2", f"every operand {nm}")
        l = V._f2s(r.operands[1])
        assert V._add_nr(l[0], l[1]) == V._add_nr(l[1], l[2]) == want
    # the bound fault of the issue: fp2_add_nr(l2, l3) instead of fp2_add pushes the second
    # fp6_mul_01's d0 + d1 to 3p - 3 on the all-p-1 record
    l = V._f2s(_rec("fp12_mul_line", "every operand p-1").operands[1])
    assert max(V._add_nr(l[0], V._add_nr(l[1], l[2]))) == 3 * P - 3


def test_frobenius_references():
    """conj(c_k) xi^(k(p-1)/6) is a^p and c_k xi^(k(p^2-1)/6) is a^(p^2), on two records"""
    recs = V.OPS["fp12_frob"].records
    for rec in (recs[-1], _rec("fp12_frob", "operand 0 (f12) p-1, the others random")):
        a = V.element("f12", rec.operands[0])
        assert V.ref_frob(a) == O.f12_pow(a, P) == O.f12_frob(a)
        assert V.ref_frob2(a) == O.f12_pow(a, P * P) == V.ref_frob(V.ref_frob(a))


def test_cyclotomic_inputs():
    ins = V.cyclotomic_inputs()
    assert ins[0][1] == tuple(O.F12_ONE) and len(ins) == 11
    for nm, c in ins:
        c = list(c)
        # in the cyclotomic subgroup: c^(p^4 - p^2 + 1) = 1, i.e. frob^4(c) c = frob^2(c)
        f2 = V.ref_frob2(c)
        assert O.f12_mul(V.ref_frob2(f2), c) == f2, nm
        assert O.f12_mul(c, O.f12_conj(c)) == O.F12_ONE, nm  # unitary
    order_r = list(ins[-1][1])
    assert order_r != O.F12_ONE and O.f12_pow(order_r, O.R) == O.F12_ONE
    assert list(ins[-2][1]) == O.f12_pow(list(ins[1][1]), O.R) != O.F12_ONE
    assert V.ref_exp_x(order_r) == O.f12_conj(O.f12_pow(order_r, O.X_ABS))


def test_line_restatement_against_the_oracles_miller_loop():
    """the restated steps' lines, multiplied in ml_f's order and conjugated, give the value that
    COP_MILLER's reference accepts for the same (RP, HQ): equal after the final exponentiation"""
    items = V.line_items()
    assert {it[1] == 1 for it in items} == {True, False}
    assert len(V.line_event_names()) == V.LINE_EVENTS
    assert sum(n.startswith("addition") for n in V.line_event_names()) == 5
    for pa, _z, q in (items[0], items[1]):
        f = V.lines_to_f(V.ref_lines(pa, q))
        assert O.final_exponentiation(f, 3) == O.final_exponentiation(O.miller_loop(pa, q), 3)
    # the check accepts the reference laid out as the op returns it and names a wrong word
    it = items[2]
    words = [w for ln in V.ref_lines(it[0], it[2]) for w in C.pack_f2s(*ln)]
    assert len(words) == 72 * V.LINE_EVENTS and V.check_lines(it, words) is None
    bad = list(words)
    bad[72 * 5 + 30] ^= 4
    assert "line 5 (doubling at bit 59) l2.c0" in V.check_lines(it, bad)  # dbl 62, add 62, dbl 61, dbl 60, add 60
    bad = list(words)
    bad[72 * 67: 72 * 67 + 12] = V.limbs(P)
    assert "not canonical" in V.check_lines(it, bad)


# ---- the same records through the host build ---------------------------------------------------
def _raw_bytes(raw) -> bytes:
    return b"".join(v.to_bytes(48, "little") for v in raw)


def _raw_words(buf: bytes, n: int) -> list[int]:
    return [int.from_bytes(buf[4 * k: 4 * k + 4], "little") for k in range(12 * n)]


def _el_bytes(el) -> bytes:
    return b"".join(f2b(c) for c in el)


def _el_words(buf: bytes) -> list[int]:
    return V.pack([V.raw_f12([bf2(buf[96 * k: 96 * k + 96]) for k in range(6)])])


def _run_host(hostsim, name, rec):
    o = ctypes.create_string_buffer(1152)
    ops = rec.operands
    if name in ("fp6_mul", "fp6_mul_01", "fp6_mul_1"):
        getattr(hostsim, "hs_" + name)(_raw_bytes(ops[0]), _raw_bytes(ops[1]), o)
        return _raw_words(o.raw, 6)
    if name == "fp6_inv":
        hostsim.hs_fp6_inv(_raw_bytes(ops[0]), o)
        return _raw_words(o.raw, 6)
    if name == "fp12_cyclotomic_exp_x":
        hostsim.hs_fp12_cyclotomic_exp_x(_raw_bytes(ops[0]), o)
        return _raw_words(o.raw, 12)
    els = [V.element(k, raw) for k, raw in zip(V.OPS[HOST_RUNS[name]].kinds, ops)]
    a = _el_bytes(els[0])
    if name in ("fp12_mul", "mul12m_conj"):
        hostsim.hs_fp12_mul(a, _el_bytes(O.f12_conj(els[1]) if name == "mul12m_conj" else els[1]), o)
    elif name in ("fp12_sqr", "fp12_inv", "fp12_frob", "fp12_frob2", "fp12_cyclotomic_sqr"):
        getattr(hostsim, "hs_" + name)(a, o)
    elif name in ("fp12_mul_line", "fp12_mul_line_pair"):
        l0, _z, l2, l3 = els[1][:4]
        getattr(hostsim, "hs_" + name)(a, f2b(l0), f2b(l2), f2b(l3), o)
    elif name == "fp12_sqr_pair":
        hostsim.hs_fp12_sqr_pair(a, o)
    elif name == "fp12_mul_line2":
        ln = [b"".join(f2b(c) for c in (e[0], e[2], e[3])) for e in els[1:]]
        hostsim.hs_fp12_mul_line2(a, ln[0], ln[1], o)
    else:
        raise KeyError(name)
    return _el_words(o.raw[:576]) + (_el_words(o.raw[576:]) if name.endswith("_pair") else [])


# host export -> the op whose records and check it gets
HOST_RUNS = {
    "fp6_mul": "fp6_mul", "fp6_mul_01": "fp6_mul_01", "fp6_mul_1": "fp6_mul_1", "fp6_inv": "fp6_inv",
    "fp12_mul": "fp12_mul", "mul12m_conj": "mul12m_conj", "fp12_sqr": "fp12_sqr", "fp12_mul_line": "fp12_mul_line",
    "fp12_inv": "fp12_inv", "fp12_frob": "fp12_frob", "fp12_frob2": "fp12_frob2",
    "fp12_cyclotomic_sqr": "cyc_sqr", "fp12_cyclotomic_exp_x": "exp_x_m", "fp12_mul_line2": "fp12_mul_line2",
    "fp12_sqr_pair": "sqr12_pair", "fp12_mul_line_pair": "mul_line12_pair",
}


@pytest.mark.parametrize("export", list(HOST_RUNS))
def test_records_against_hostsim(hostsim, export):
    """the CPU build of the same header function on every record of the op, through the check
    the GPU output gets; and the check is not vacuous: one flipped bit of a word is refused"""
    t = V.OPS[HOST_RUNS[export]]
    bad = 0
    for i, rec in enumerate(t.records):
        out = _run_host(hostsim, export, rec)
        err = t.check(rec, out)
        assert err is None, V.failure(t, t.flavours[0], i, rec, "host build: " + err)
        if i % 7 == 0:
            flipped = list(out)
            flipped[len(out) - 7 - 12 * (i % 5)] ^= 1 << 9
            bad += t.check(rec, flipped) is not None
    assert bad == len(range(0, len(t.records), 7)), export
    rec = t.records[-1]
    out = _run_host(hostsim, export, rec)
    err = t.check(rec, V.limbs(P) + out[12:])
    assert err is not None and "not canonical" in err
