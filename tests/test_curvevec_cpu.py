"""The curve-op self-test's vectors and references (tests/_curvevec.py) checked on the CPU:
every set's reference is self-consistent (points on their curves, u and -u, [h_eff]P,
H(m)), the directed inputs really sit on the branches they are meant for, and the same
records through the CPU build of the same headers (tests/native/hostsim.cpp) pass the very
checks the GPU output gets -- so a wrong reference or a malformed record shows here, before
any GPU run.  (What the device compiles differently -- the 32-bit column product, the
28-bit-digit one, the out-of-line Fp2 primitive under k_chain's role 0 -- is what
tests/test_gpu_curve_ops.py then runs.)"""
from __future__ import annotations

import ctypes

import pytest

from oracle import bls_oracle as O
from tests import _curvevec as V
from tests import _groupedge as ge
from tests._codec import P, b48, bf2, bg2, f2b, fp, g2b


def test_case_list_and_library_shapes():
    """every record packs to the op's input size in the C table; an op is refused in the
    flavour it does not exist in, and past the table"""
    from lodestar_amd._abi import load_library

    lib = load_library()
    iw, ow = ctypes.c_uint32(), ctypes.c_uint32()
    assert len(V.SETS) == V.N_OPS and sorted(s.op for s in V.SETS.values()) == list(range(V.N_OPS))
    assert len(V.CASES) == 10
    for s in V.SETS.values():
        recs = s.records()
        assert 0 < len(recs) < 400, s.name
        for fl in (0, V.D28):
            rc = lib.bls_gpu_curve_op_shape(s.op | fl, ctypes.byref(iw), ctypes.byref(ow))
            assert rc == (0 if fl in s.flavours else -2), (s.name, fl)
            if rc == 0:
                for rec in recs:
                    w = s.pack(rec)
                    assert len(w) == iw.value and all(0 <= x < 1 << 32 for x in w), s.name
    for op, shape in ((V.MILLER, (86, 144)), (V.FE, (144, 2))):
        assert lib.bls_gpu_curve_op_shape(op, ctypes.byref(iw), ctypes.byref(ow)) == -2
        assert lib.bls_gpu_curve_op_shape(op | V.D28, ctypes.byref(iw), ctypes.byref(ow)) == 0
        assert (iw.value, ow.value) == shape
    assert len(V.pack_miller(V.miller_items()[0], 2)) == 86 and len(V.f12_pack(V.fe_tasks()[0][1])) == 144
    assert lib.bls_gpu_curve_op_shape(V.FE + 1, ctypes.byref(iw), ctypes.byref(ow)) == -2
    assert lib.bls_gpu_curve_op_shape((V.FE + 1) | V.D28, ctypes.byref(iw), ctypes.byref(ow)) == -2
    assert lib.bls_gpu_curve_op_shape(0x200, ctypes.byref(iw), ctypes.byref(ow)) == -2


def test_from_be64_and_h2f_inputs():
    vals = V.from_be64_values()
    top = 1 << 512
    q = top // P * P
    for v in (0, 1, P - 1, P, P + 1, (1 << 256) - 1, ((1 << 256) - 1) << 256, 1 << 256, top - 1, q - 1, q, q + 1):
        assert v in vals
    assert q % P == 0 and q + P > top and len(vals) == 12 + 32
    assert V.pack_be64(1)[15] == 1 and V.pack_be64(1 << 511)[0] == 1 << 31
    msgs = V.h2f_messages()
    assert msgs[0] == bytes(32) and msgs[1] == b"\xff" * 32 and len(msgs) == 10 + 64
    for k in range(8):
        w = V.pack_msg(msgs[2 + k])
        assert bin(w[k]).count("1") == 1 and not any(w[j] for j in range(8) if j != k)


def test_c1_zero_inputs():
    """the u whose g(x1) lies in Fp: at least 8, both kinds, and really on that branch"""
    us = V.c1_zero_us()
    assert len(us) >= 8
    pick = V.c1_zero_pick()
    kinds = [k for u, k in us if u in pick]
    assert len(pick) >= 8 and kinds.count(True) >= 2 and kinds.count(False) >= 2
    for u in pick:
        den, sq, g = V.sswu_gx(u)
        assert not O.f2_is_zero(den) and sq and g[1] == 0
        y = V.ref_sswu(u)[1]
        real = O.legendre(g[0]) == 1
        assert (y[1] == 0 and y[0] != 0) if real else (y[0] == 0 and y[1] != 0)  # purely imaginary: sgn0 from c1


def test_sswu_reference_and_branches():
    directed, rand = V.sswu_inputs()
    for v in (1, 2, P - 1, P - 2):
        assert (v, 0) in directed and (0, v) in directed
    assert (0, 0) in directed and (P - 1, P - 1) in directed
    for u in directed:
        x, y = V.ref_sswu(u)
        assert O.E2_ISO.on_curve((x, y))
        assert O.f2_neg(u) in directed
        if u != (0, 0):
            assert V.ref_sswu(O.f2_neg(u)) == (x, O.f2_neg(y))
    # the fast map refuses u = 0 and the g(x1) in Fp set, nothing else
    refused = {u for u in V.sswu_us() if not V.fast_ok(u)}
    c1 = set(V.c1_zero_pick())
    assert refused == {(0, 0)} | c1 | {O.f2_neg(u) for u in c1}
    assert O.f2_is_zero(V.sswu_x1((0, 0))[0])
    assert all(V.fast_ok(u) for u in rand) and len(rand) == 200
    # outer branch: g(x1) a square or not.  Inner branch: d = (g.c0 + gamma) / 2 a square
    # or not, gamma^2 = N(g); d d' = -(g.c1 / 2)^2 is a non-square, so exactly one sign of
    # gamma makes d a square.  Where g(x1) is a square the map's gamma is N^((p+1)/4);
    # where it is not, gamma carries the sign of the constant sqrt(-125), which the oracle
    # does not fix: the count must hold for either.
    outer = {True: 0, False: 0}
    inner_sq = {True: 0, False: 0}
    for u in rand:
        _den, sq, g = V.sswu_gx(u)
        outer[sq] += 1
        gamma = pow((g[0] * g[0] + g[1] * g[1]) % P, (P + 1) // 4, P)
        inner_sq[sq] += O.legendre((g[0] + gamma) * pow(2, -1, P) % P) == 1
    assert min(outer.values()) >= 50, outer
    k, m = inner_sq[False], outer[False]
    for flip in (k, m - k):
        d_square = inner_sq[True] + flip
        assert min(d_square, len(rand) - d_square) >= 50, (inner_sq, outer)


def test_iso_reference():
    """the x-denominator is (x - r)^2 and the y-denominator (x - r)^3: one pole in all"""
    poles = V.iso_poles()
    assert len(poles) == 1
    r = poles[0]
    two_r = O.f2_muls(r, 2)
    assert O.ISO_XDEN == [O.f2_sqr(r), O.f2_neg(two_r), O.F2_ONE]
    assert O.ISO_YDEN == [O.f2_neg(O.f2_mul(O.f2_sqr(r), r)), O.f2_muls(O.f2_sqr(r), 3), O.f2_muls(O.f2_neg(r), 3),
                          O.F2_ONE]
    pts = V.iso_inputs()
    n_pole = len(V.pole_points())
    assert n_pole == 2
    for q in pts[-n_pole:]:
        assert O.iso_map(q) is None
    for q in pts[:-n_pole]:
        assert O.E2_ISO.on_curve(q)
        im = O.iso_map(q)
        assert im is not None and O.E2.on_curve(im)
    assert V.jac_to_affine([3, 4, 5, 6, 0, 0]) is None
    x, y = pts[0]
    z = (7, 9)
    z2 = O.f2_sqr(z)
    assert V.jac_to_affine([*O.f2_mul(x, z2), *O.f2_mul(y, O.f2_mul(z2, z)), *z]) == (x, y)


def test_clear_cofactor_reference():
    recs = V.clear_inputs()
    names = [nm for nm, _ in recs]
    assert names[0] == "infinity" and sum(nm.startswith("iso(") for nm in names) == 32
    for nm, pt in recs:
        want = V.ref_clear(pt)
        assert O.E2.on_curve(pt) and want == O.E2.mul(pt, O.H_EFF), nm
        assert want is None or O.g2_in_subgroup(want), nm
        if nm.startswith("order 13") or nm == "infinity":
            assert want is None, nm
        if nm.startswith("order 23"):  # the control of tests/_groupedge.py: off G2, of order 23
            assert O.E2.mul(pt, 23) is None and not O.g2_in_subgroup(pt)
    assert ge.H2 % 13 == 0  # why [h_eff] kills the order-13 point


def test_chain_h_reference():
    recs = {nm: (q0, q1) for nm, q0, q1 in V.chain_directed()}
    q0, q1 = recs["q1 == q0 (doubling)"]
    assert q0 == q1 and V.ref_chain_h(q0, q1) == O.clear_cofactor_g2(O.E2.dbl(O.iso_map(q0)))
    q0, q1 = recs["q1 == -q0 (H = O)"]
    assert O.E2.add(O.iso_map(q0), O.iso_map(q1)) is None and V.ref_chain_h(q0, q1) is None
    for k in range(2):
        q0, q1 = recs[f"q0 at pole ({k}), q1 ordinary"]
        assert O.iso_map(q0) is None and V.ref_chain_h(q0, q1) == O.clear_cofactor_g2(O.iso_map(q1)) is not None
    q0, q1 = recs["q0 ordinary, q1 at pole"]
    assert V.ref_chain_h(q0, q1) == O.clear_cofactor_g2(O.iso_map(q0))
    assert V.ref_chain_h(*recs["both at the pole"]) is None and V.ref_chain_h(*recs["both at the pole, same y"]) is None
    # the fed-forward records' expectation: the verify path's H is hash_to_g2 of the message
    for m in V.chain_messages()[:6]:
        u0, u1 = O.hash_to_field_fp2(m, 2, O.DST_POP)
        assert V.ref_chain_h(V.ref_sswu(u0), V.ref_sswu(u1)) == O.hash_to_g2(m)
    # the check accepts the exact answer and refuses one flipped bit, a wrong byte, a written HQ at H = O
    for nm, q0, q1 in V.chain_directed():
        want = V.ref_chain_h(q0, q1)
        out = [1] + [0] * 48 if want is None else [0] + V.pack_fps(V._flat(want))
        assert V.check_chain_h(want, out) is None, nm
        bad = list(out)
        bad[17] ^= 1 << 3
        assert V.check_chain_h(want, bad) is not None, nm
        assert V.check_chain_h(want, [out[0] ^ 1] + out[1:]) is not None, nm
    assert V.check_chain_h((q0, q1), [0] + V.limbs(P) + [0] * 36) is not None  # not canonical


# ---- the same records through the host build ---------------------------------------------------
def _mont_words(raw: bytes, n: int):
    return [w for k in range(n) for w in V.limbs(V.mont(fp(raw[48 * k: 48 * k + 48])))]


def _run_host(hostsim, name, rec):
    """output words of set `name`'s record through the hostsim export of the same function"""
    o = ctypes.create_string_buffer(384)
    if name == "from_be64":
        hostsim.hs_fp_from_be64_words((ctypes.c_uint32 * 16)(*V.pack_be64(rec)), o)
        return _mont_words(o.raw, 1)
    if name == "h2f":
        hostsim.hs_hash_to_field(rec, o)
        return _mont_words(o.raw, 4)
    if name == "sswu":
        hostsim.hs_map_to_curve_sswu(f2b(rec), o)
        return _mont_words(o.raw, 4)
    if name == "sswu_fast":
        ok = hostsim.hs_map_to_curve_sswu_fast(f2b(rec), o)
        return [int(ok)] + (_mont_words(o.raw, 4) if ok else [0] * 48)
    if name == "iso_aff":
        ok = hostsim.hs_iso_map_g2(f2b(rec[0]) + f2b(rec[1]), o)
        return [int(not ok)] + (_mont_words(o.raw, 4) if ok else [0] * 48)
    if name == "iso_jac":  # the export returns the affine point: Z = 1
        ok = hostsim.hs_iso_map_jac(f2b(rec[0]) + f2b(rec[1]), o)
        return (_mont_words(o.raw, 4) + V.pack_fps([1, 0])) if ok else V.pack_fps([1, 0, 1, 0, 0, 0])
    if name == "clear_cofactor":
        hostsim.hs_g2_clear_cofactor(g2b(rec[1]), o)
        pt = bg2(o.raw[:192])
        return V.pack_point(pt)
    raise KeyError(name)


HOST_SETS = ("from_be64", "h2f", "sswu", "sswu_fast", "iso_aff", "iso_jac", "clear_cofactor")


@pytest.mark.parametrize("name", HOST_SETS)
def test_vectors_against_hostsim(hostsim, name):
    """includes the first call of hs_g2_clear_cofactor and fp_from_be64_words off SHA output"""
    s = V.SETS[name]
    bad = 0
    for i, rec in enumerate(s.records()):
        out = _run_host(hostsim, name, rec)
        err = s.check(rec, out)
        assert err is None, V.failure(s, s.flavours[0], i, rec, "host build: " + err)
        if i < 12:  # the check is not vacuous: one flipped bit of a value word is refused
            flipped = list(out)
            flipped[len(out) - 7] ^= 1 << 9
            bad += s.check(rec, flipped) is not None
    assert bad >= 8, name


# ---- Miller loops and final exponentiations ----------------------------------------------------------
def test_miller_layout_has_full_and_partial_groups():
    items = V.miller_items()
    doms = [it[3] for it in items]
    assert sorted(set(V.DOMAIN_SIZES)) == [1, 2, 3, 4, 5] and len(items) == sum(V.DOMAIN_SIZES) == 27
    assert {it[1] == 1 for it in items} == {True, False}          # z = 1 and a random z
    assert all(O.E1.on_curve(it[0]) and O.g2_in_subgroup(it[2]) for it in items)
    for pl in (2, 4):
        holds = V.miller_shared(pl, doms)
        sizes = [len(v) for v in holds.values()]
        assert pl in sizes and 1 in sizes and sizes.count(0) >= pl - 1  # whole groups, items alone, exact ones
        for k0, grp in holds.items():
            assert len({doms[i] for i in grp}) <= 1
    assert 3 in [len(v) for v in V.miller_shared(4, doms).values()]    # the odd tail of a shared loop
    for pl in (1, V.MLF_PAIR):
        assert V.miller_shared(pl, doms) == {i: [i] for i in range(27)}


def _host_miller(hostsim, item):
    pa, z, q, _d = item
    o = ctypes.create_string_buffer(576)
    hostsim.hs_miller_loop_jac(O.g1_serialize(pa), b48(z), g2b(q), o)
    return [bf2(o.raw[96 * k: 96 * k + 96]) for k in range(6)]


def test_miller_vectors_against_hostsim(hostsim):
    """the check accepts the host build's Miller values laid out as each items-per-lane
    leaves them (a shared f in the group's first item, 1 in the others), and refuses a
    wrong f, a missing 1 and a non-canonical word"""
    items = V.miller_items()
    fs = [_host_miller(hostsim, it) for it in items]
    doms = [it[3] for it in items]
    for pl in V.PER_LANES:
        holds = V.miller_shared(pl, doms)
        rows = [V.f12_pack(V.f12_prod([fs[j] for j in holds[i]])) for i in range(len(items))]
        assert V.check_miller(pl, rows, "host") is None
    bad = [list(r) for r in rows]
    bad[9][30] ^= 1
    assert "domain 2" in V.check_miller(V.MLF_PAIR, bad, "host")
    holds = V.miller_shared(4, doms)
    rows = [V.f12_pack(V.f12_prod([fs[j] for j in holds[i]])) for i in range(len(items))]
    rows[2] = V.f12_pack(fs[2])
    assert "exactly 1" in V.check_miller(4, rows, "host")
    rows[2] = V.limbs(P) + [0] * 132
    assert "not canonical" in V.check_miller(4, rows, "host")
    # bilinearity of the reference itself
    a, b = V.bilinear_items()
    assert O.final_exponentiation(O.miller_loop(a[0], a[2]), 3) == O.final_exponentiation(O.miller_loop(b[0], b[2]), 3)


def test_fe_tasks_against_hostsim(hostsim):
    tasks = V.fe_tasks()
    want = [V.ref_fe_is_one(k) for k in range(len(tasks))]
    assert want[:7] == [True] * 7 and want[7:10] == [False] * 3 and want[16:] == [True] * 3 and len(tasks) == 19
    for _nm, f in tasks[16:]:  # FE = 1 although the easy part's value is not 1
        assert not O.f12_is_one(O.f12_pow(list(f), O.FE_EASY))
    o = ctypes.create_string_buffer(576)
    for k, (nm, f) in enumerate(tasks):
        hostsim.hs_final_exp(b"".join(f2b(c) for c in f), o)
        got = [bf2(o.raw[96 * j: 96 * j + 96]) for j in range(6)]
        assert got == O.final_exponentiation(list(f), 3), nm
        assert V.f12_unpack([V.unmont(v) for v in V.raw_fps(V.f12_pack(f), 12)]) == list(f)
