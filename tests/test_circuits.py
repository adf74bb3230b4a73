"""The cooperative-kernel programs (tools/gen_coop.py), simulated with the device's
step semantics (tools/circuits.py:simulate), against the oracle's math.  CPU only."""
from __future__ import annotations

import random
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import gen_coop as GC  # noqa: E402
from circuits import P, simulate  # noqa: E402

from tests._coopsim import CoopTable  # noqa: E402


@pytest.fixture(scope="module")
def progs(coop_programs):
    return coop_programs


def put12(frame, base, f):
    # oracle w-basis coefficients [c0..c5] -> struct order A(c0,c2,c4), B(c1,c3,c5)
    for k in range(2):
        for j in range(3):
            c = f[2 * j + k]
            frame[base + 6 * k + 2 * j] = c[0]
            frame[base + 6 * k + 2 * j + 1] = c[1]


def get12(frame, base):
    return [(frame[base + 6 * (w % 2) + 2 * (w // 2)], frame[base + 6 * (w % 2) + 2 * (w // 2) + 1])
            for w in range(6)]


def rand12(rng):
    return [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]


def to_jac(pt, z):
    (x, y) = pt
    z2 = z
    zz = [(z2[0] * z2[0] - z2[1] * z2[1]) % P, 2 * z2[0] * z2[1] % P]
    from oracle.bls_oracle import f2_mul
    zz = f2_mul(z, z)
    zzz = f2_mul(zz, z)
    return f2_mul(x, zz), f2_mul(y, zzz), z


def test_fin_fmul(progs, oracle):
    pg, consts = progs
    rng = random.Random(1)
    fr = [0] * GC.FRAME
    a, b = rand12(rng), rand12(rng)
    put12(fr, GC.F, a)
    put12(fr, GC.G, b)
    simulate(pg["fin_fmul"], fr, consts)
    assert get12(fr, GC.F) == oracle.f12_mul(a, b)


def test_fin_final_exponentiation(progs, oracle):
    pg, consts = progs
    rng = random.Random(3)
    q = oracle.E2.mul(oracle.G2, rng.randrange(1, 1 << 64))
    pp = oracle.E1.mul(oracle.G1, rng.randrange(1, 1 << 64))
    f0 = oracle.f12_mul(rand12(rng), oracle.miller_loop(pp, q))
    fr = [0] * GC.FRAME
    put12(fr, GC.F, f0)
    simulate(pg["fin_fe1"], fr, consts)
    fr[GC.INV_OUT] = pow(fr[GC.INV_IN], P - 2, P)
    simulate(pg["fin_fe2"], fr, consts)
    assert get12(fr, GC.F) == oracle.final_exponentiation(f0, hard_multiple=3)


def test_emitted_lane_groups_match_program(progs, tmp_path):
    """Steps with spare lanes spread their products and combinations over lane groups of
    2 or 4 (gen_coop.lane_entries); the table the device runs computes what the program
    does."""
    pg, consts = progs
    path = tmp_path / "t.bin"
    # pset_phase2 / pset2_phase2 / pset3_phase2 hold the subgroup test's combination-only
    # steps (psi(sig) - [x] sig into PS_DIFF, k_pset.hip's BLST_POINT_NOT_IN_GROUP test): the
    # round-5 GPU failure gpurun_out/r5i/pytest.log (-3 for a valid signature on the 1-set
    # path: a wrong PS_DIFF) came from an uncommitted first form of the lane-pair
    # combinations; every program the device runs with lane groups is
    # checked here
    names = ["pset_dbl_all", "pset_add_x", "fin_fe1", "fin_fmul", "pset_norm2", "pset_ml2_w2", "pset_xchain",
             "fin_fe2_w2", "pset_prep", "pset_phase2", "pset_affine2", "pset2_phase2", "pset3_phase2", "pset3_prep",
             "ml1_1", "ml1_2"]
    GC.emit([pg[nm] for nm in names], consts, path)
    sizes = [GC.lane_entries(st, getattr(pg[nm], "lanes", 64))[1:] for nm in names for st in pg[nm].steps]
    assert sum(gp == 2 for gp, _ in sizes) >= 10 and sum(gp == 4 for gp, _ in sizes) >= 3
    assert sum(gl == 4 for _, gl in sizes) >= 5
    rng = random.Random(7)
    table = CoopTable.from_file(path)  # tests/_coopsim.py: coop.hpp coop_step's semantics, lane by lane
    for nm in names:
        fr = [rng.randrange(P) for _ in range(pg[nm].n_slots)]
        fr2 = list(fr)
        f1 = simulate(pg[nm], fr, consts)
        f2 = table.run(nm, fr2)
        assert (fr, f1) == (fr2, f2), nm


def test_emitted_accumulators_within_acc_reduce_bound(progs, tmp_path):
    """acc_reduce's precondition (coop.hpp), which nothing else checks: the accumulator
    it reduces is a sum of c x over values x < 3p, and the 2^20 p bias makes it
    non-negative only while sum |c| * 3 <= 2^20; every |c| fits the int16 field with
    room (|c| < 2^15).  Over every accumulator of the emitted table: one lane's operand,
    or the operands the DPP butterflies add together (the gl lanes of a combination
    group, each half of a product group)."""
    pg, consts = progs
    path = tmp_path / "all.bin"
    GC.emit(list(pg.values()), consts, path)
    table = CoopTable.from_file(path)
    assert set(table.programs) == set(pg)
    n_acc, worst_sum, worst_c = 0, 0, 0
    for nm in table.programs:
        for cs in table.accumulators(nm):
            n_acc += 1
            assert all(abs(c) < 1 << 15 for c in cs), (nm, cs)
            assert 3 * sum(abs(c) for c in cs) <= 1 << 20, (nm, cs)
            worst_sum = max(worst_sum, sum(abs(c) for c in cs))
            worst_c = max([worst_c] + [abs(c) for c in cs])
    assert n_acc > 10000 and worst_c > 1  # (the real table: largest sum |c| 147, largest |c| 144)
