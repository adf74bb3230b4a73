"""Device-only arithmetic, unit by unit, on the GPU against Python integers.

What the GPU executes for the field is not what the CPU harness compiles: the carry
chains are inline asm (bls/carry_asm.hpp), the 28-bit-digit products run ordered
v_mad_u64_u32 / v_mad_i64_i32 blocks, the 32-bit column product and the interpreter's
accumulator (bls/coop.hpp coop_lin_acc, acc_reduce, the DPP butterflies,
fp_is_zero_lazy) exist on the device only.  Two entry points reach them directly:

* bls_gpu_field_op_test: one primitive per launch on raw operands, edges included
  (vectors and exact references: tests/_fieldvec.py, checked on the CPU by
  tests/test_fieldvec.py).  A failure names the primitive and the operand.
* bls_gpu_coop_run_test: every program of the table the library loaded, run once on
  frames of lazy representatives, against the table's reference interpreter
  (tests/_coopsim.py): every slot below 3p and congruent, the flag word equal.
"""
from __future__ import annotations

import functools
import random
from pathlib import Path

import numpy as np
import pytest

from tests import _fieldvec as V
from tests._codec import P
from tests._coopsim import CoopTable

pytestmark = pytest.mark.gpu

TABLE_PATH = Path(__file__).resolve().parent.parent / "lodestar_amd" / "_native" / "coop_tables.bin.gz"
R = 1 << 384
R_INV = pow(R, -1, P)


@pytest.mark.parametrize("name,flavour", V.CASES, ids=[f"{nm}-{'d28' if fl else 'cols'}" for nm, fl in V.CASES])
def test_field_op(gpu, name, flavour):
    """one launch: every record of the op's vector set through the primitive, raw words in and out"""
    s = V.sets()[name]
    recs = np.array([s.pack(r) for r in s.records], dtype=np.uint32)
    out = gpu.field_op_test(s.op | flavour, recs)
    assert out.shape[0] == len(s.records)
    tu = "k_selftest_d28" if flavour else "k_selftest"
    for i, rec in enumerate(s.records):
        err = s.check(rec, [int(w) for w in out[i]])
        assert err is None, f"{tu} record {i}: {err}"


def test_field_op_unknown_is_refused(gpu):
    from lodestar_amd.native import NativeError

    for op in (V.PREDS + 1, V.CANON3, V.LIN8, 0x200):  # past the table; d28-only ops without the flag
        with pytest.raises(NativeError):
            gpu.field_op_shape(op)


# ---- the interpreter, program by program, against the table it loaded ----------------------
@functools.lru_cache(maxsize=None)
def _table():
    return CoopTable.from_file(TABLE_PATH)  # the very bytes the library loaded, parsed once


@pytest.fixture(scope="module")
def table():
    return _table()


def _program_names():
    # (at collection: the table is there once the library is built; without it the
    # parametrisation is empty and the guard test below fails)
    return list(_table().programs) if TABLE_PATH.exists() else []


def test_table_is_the_built_one(table):
    assert _program_names() == list(table.programs) and len(table.programs) >= 29


def _frames(name: str, n_slots: int):
    """four frames of plain residues with the representative k of each slot (device value
    = Montgomery form + k p): random canonical; the same residues as lazy representatives;
    one residue everywhere (the exact reference then sets zero-check flags and leaves many
    slots congruent to 0: the exact-multiple case of acc_reduce, the p / 2p case of
    fp_is_zero_lazy) with mixed representatives; every slot 3p - 1"""
    rng = random.Random("coop-run-" + name)
    res = [rng.randrange(P) for _ in range(n_slots)]
    v = rng.randrange(1, P)
    top = (3 * P - 1) * R_INV % P  # the residue whose Montgomery form + 2p is 3p - 1
    assert top * R % P + 2 * P == 3 * P - 1
    return [(res, [0] * n_slots), (res, [rng.randrange(3) for _ in range(n_slots)]),
            ([v] * n_slots, [rng.randrange(3) for _ in range(n_slots)]), ([top] * n_slots, [2] * n_slots)]


@pytest.mark.parametrize("name", _program_names())
def test_coop_program_matches_table(gpu, table, name):
    n_slots = table.n_slots(name)
    frames = _frames(name, n_slots)
    raw = np.zeros((len(frames), n_slots, 12), dtype=np.uint32)
    for f, (res, ks) in enumerate(frames):
        for sl in range(n_slots):
            val = res[sl] * R % P + ks[sl] * P
            assert val < 3 * P
            raw[f, sl] = V.limbs(val)
    out, flags = gpu.coop_run_test(name, raw)
    for f, (res, _ks) in enumerate(frames):
        want = list(res)
        want_flag = table.run(name, want)
        for sl in range(n_slots):
            got = V.unlimbs(out[f, sl])
            assert got < 3 * P, f"{name} frame {f} slot {sl}: {got:#x} is not below 3p"
            assert got * R_INV % P == want[sl], f"{name} frame {f} slot {sl}: {got:#x}, want {want[sl] * R % P:#x} (mod p)"
        assert int(flags[f]) == want_flag, f"{name} frame {f}: flag word {int(flags[f]):#x}, want {want_flag:#x}"
    if name.endswith("_prep"):  # the all-equal frame sets every packed set's zero-check flag
        sets = {"pset_prep": 1, "pset2_prep": 3, "pset3_prep": 7}[name]
        assert int(flags[2]) == sets


def test_coop_run_rejects_wrong_frame_size(gpu, table):
    from lodestar_amd.native import NativeError

    with pytest.raises(NativeError):
        gpu.coop_run_test("pset2_prep", np.zeros((1, 256, 12), dtype=np.uint32))  # its frame is 380 slots
    with pytest.raises(NativeError):
        gpu.coop_run_test("no_such_program", np.zeros((1, 256, 12), dtype=np.uint32))


def test_coop_probe_finds_its_program_as_the_run_test_does(gpu, table):
    """bls_gpu_coop_probe looks its program up as bls_gpu_coop_run_test does: a known name is
    timed (and stamped: 2 * steps + 1 words, none lost behind the blocks' sink), an unknown
    one is "no program ..." from both."""
    from lodestar_amd.native import NativeError

    n_steps = table.programs["fin_fmul"][1]
    us, ms, stamps = gpu.coop_probe("fin_fmul", 3, 1, 2 * n_steps + 1)
    assert us > 0 and ms > 0 and stamps.shape == (2 * n_steps + 1,)
    assert all(int(t) != 0 for t in stamps[1:]), "every step of the stamped run starts and ends"
    for call in (lambda: gpu.coop_probe("no_such_program", 1, 1),
                 lambda: gpu.coop_run_test("no_such_program", np.zeros((1, 256, 12), dtype=np.uint32))):
        with pytest.raises(NativeError, match="no program no_such_program"):
            call()


def test_timing_probes_run_and_report(gpu):
    """The other timing probes have no output to compare: each runs to its end on a small
    shape and reports a time, and an unknown design probe is refused."""
    from lodestar_amd.native import NativeError

    ns, rate = gpu.fpm_bench(1024, 64)
    assert ns > 0 and rate > 0
    assert gpu.kernel_probe("fpm_d28", 65, 2) > 0
    assert gpu.mad_peak()[0] > 0
    with pytest.raises(NativeError, match="unknown probe"):
        gpu.kernel_probe("no_such_probe", 64, 1)
