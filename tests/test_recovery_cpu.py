"""The recovery sweep (tests/_recovery.py) on the CPU: the builder holds every case it is
meant to hold, its model of the group-test rounds gives the oracle's verdicts, and the
model's pass A is the planner's (bls/plan.hpp plan_group_tests_a and bls/group_decode.hpp,
compiled into libhostsim.so) -- the tests, the whole / chunk-check choice and the decoded
request, for all three $BLS_GROUP_EQ modes with the chunk-check value kept and not kept.
The GPU side is tests/test_gpu_recovery.py."""
from __future__ import annotations

import ctypes
import random
from collections import Counter

import pytest

import _recovery as R
from test_plan_cpu import NONE, REF_CHUNK, _call, _i32, _u32


@pytest.fixture(scope="module")
def lists():
    return {"sweep": R.sweep(), "structure": R.structure()}


def test_sweep_holds_every_case(lists):
    sweep = lists["sweep"]
    fam = Counter(m["family"] for m in sweep)
    by = lambda f: [m for m in sweep if m["family"] == f]  # noqa: E731
    # single invalid request: every position of every m, both sides of every nbits step
    singles = by("single")
    assert sorted((m["m"], m["bad"][0]) for m in singles) == [(m, b) for m in R.SINGLE_M for b in range(m)]
    assert R.SINGLE_M == (4, 5, 8, 9, 16, 17, 31) and fam["single"] == 90
    assert sum(len(m["reqs"]) for m in singles) == sum(m * m for m in R.SINGLE_M) == 1692
    assert sorted({R.nbits_of(m) for m in R.SINGLE_M}) == [2, 3, 4, 5]
    # pairs: all of m = 5 and m = 16, those with index 16 of m = 17; the three triples
    pairs = Counter(m["m"] for m in by("pair"))
    assert pairs == {5: 10, 16: 120, 17: 16} and fam["pair"] == 146
    assert len({(m["m"], tuple(m["bad"])) for m in by("pair")}) == 146
    assert all(m["bad"][1] == 16 for m in by("pair") if m["m"] == 17)
    assert sorted(tuple(m["bad"]) for m in by("triple")) == [(0, 1, 2), (5, 10, 15), (13, 14, 15)]
    assert all(m["m"] == 16 for m in by("triple"))
    # the OK count differs from the chunk size
    assert sorted((m["err"][0], m["bad"][0]) for m in by("shifted")) == \
        [(e, b) for e in range(9) for b in range(9) if b != e] and fam["shifted"] == 72
    assert sorted(m["err"] for m in by("err_only")) == [[e] for e in range(9)] and not any(m["bad"] for m in by("err_only"))
    assert sorted((len(m["err"]), len(m["bad"])) for m in by("survivor")) == [(3, 0)] * 4 + [(3, 1)] * 4
    assert [(m["m"], m["err"]) for m in by("all_err")] == [(4, [0, 1, 2, 3])]
    assert fam["two_survivors"] == 20 and all(m["m"] == 5 and len(m["err"]) == 3 and len(m["bad"]) == 1
                                              for m in by("two_survivors"))
    assert len({(tuple(m["err"]), m["bad"][0]) for m in by("two_survivors")}) == 20
    # neighbours: passing chunks of 4, 16 and 31, messages below gt_min valid and invalid at
    # every position, two non-batchable requests (one valid, one invalid)
    assert {m["m"] for m in by("valid")} == {4, 16, 31}
    small = {(m["m"], tuple(m["bad"])) for m in by("small")}
    assert small == {(n, ()) for n in (1, 2, 3)} | {(n, (b,)) for n in (1, 2, 3) for b in range(n)}
    nb = by("nonbatch")
    assert nb and all([b for b, _ in m["reqs"]] == [False, False] and m["bad"] == [1] for m in nb)
    # ... interleaved: no run of more than eight failing messages
    failing = len(R.sweep_failing())
    assert failing == 90 + 146 + 3 + 72 + 9 + 8 + 1 + 20 and len(sweep) == failing + failing // 8
    run = 0
    for m in sweep:
        run = 0 if m["family"] in ("valid", "small", "nonbatch") else run + 1
        assert run <= 8
    assert len({m["name"] for m in sweep}) == len(sweep)
    assert 4700 <= sum(len(t) for m in sweep for _, t in m["reqs"]) <= 5400
    assert set(fam) == {"single", "pair", "triple", "shifted", "err_only", "survivor", "all_err", "two_survivors",
                        "valid", "small", "nonbatch"}


def test_structure_holds_every_case(lists):
    st = [m for m in lists["structure"] if m["family"] == "structure"]
    seen = set()
    for m in st:
        assert len(m["reqs"]) == 16 and len(m["bad"]) == 1
        sizes = {len(t) for _, t in m["reqs"]}
        assert len(sizes) == 1
        s = sizes.pop()
        toks = m["reqs"][m["bad"][0]][1]
        assert toks.count(0) == 1 and sum(t.count(0) for _, t in m["reqs"]) == 1
        seen.add((s, m["bad"][0], toks.index(0)))
        assert m["roots"] == [i % 2 for i in range(16 * s)]
    assert seen == {(s, r, i) for s in R.STRUCT_SETS for r in (0, 15) for i in (0, s - 1)}
    assert R.STRUCT_SETS == (1, 4, 5, 16, 17)
    assert [m["name"] for m in lists["structure"] if m["family"] == "valid"] == ["struct-valid"]
    assert R.batchable_only(lists["structure"]) == lists["structure"]


def test_model_verdicts_are_the_oracles(lists, oracle):
    for name, msgs in lists.items():
        exp = R.expectations(oracle, msgs)
        for msg, e in zip(msgs, exp):
            for variant in R.VARIANTS:
                v, cnt = R.model_message(msg, variant)
                assert v == e["verdicts"], (R.describe(msg), variant)
                assert cnt == e["counters"][variant]
            assert e["counters"]["gt_off"] == [0] * 8
        # summed, as one verify_many call reports them
        retries, ok, _ = R.totals(exp, "eq1_kept")
        assert ok == sum(len(m["reqs"][r][1]) for m in msgs for pos, st in R.message_chunks(m)
                         if all(x == 1 for x in st) for r in pos)
        assert retries == sum(1 for m in msgs for _, st in R.message_chunks(m) if st and not all(x == 1 for x in st))
        assert sum(len(m["reqs"]) for m in msgs) == sum(len(e["verdicts"]) for e in exp)


def test_counters_closed_form(lists):
    """the rules of the rounds, restated per family: at most one invalid OK request is
    decided in pass A, anything else sends the m OK requests to pass C; without complement
    inference one invalid request takes pass B's two tests"""
    for msg in lists["sweep"] + lists["structure"]:
        fam, m = msg["family"], msg["m"]
        nb = R.nbits_of(m)
        got = {v: R.model_message(msg, v)[1] for v in R.VARIANTS}
        if fam in ("single", "structure"):
            assert got["eq1_kept"] == [1, 1, nb, 1, 0, 0, 0, 0], msg["name"]
            assert got["eq1_lost"] == got["eq2_kept"] == got["eq2_lost"] == [1, 0, 1 + nb, 1, 0, 0, 0, 0]
            assert got["eq0_kept"] == got["eq0_lost"] == [1, 0, nb, 0, 2, 1, 0, 0]
            assert got["gt16"] == (got["eq1_kept"] if m >= 16 else [0] * 8)
        elif fam in ("pair", "triple"):
            assert got["eq1_kept"] == [1, 1, nb, 0, 0, 0, m, 0], msg["name"]
            assert got["eq2_kept"] == [1, 0, 1 + nb, 0, 0, 0, m, 0]
            # the bit groups' OR: past m, or a request that is invalid but not alone
            idx = 0
            for b in msg["bad"]:
                idx |= b
            assert got["eq0_kept"] == [1, 0, nb, 0, 2 if idx < m else 0, 0, m, 0], msg["name"]
        elif fam == "shifted":  # m = 8 of 9, an erroneous request: always a whole test
            for v in ("eq1_kept", "eq1_lost", "eq2_kept"):
                assert got[v] == [1, 0, 4, 1, 0, 0, 0, 0], msg["name"]
            assert got["eq0_kept"] == [1, 0, 4, 0, 2, 1, 0, 0]
        elif fam == "err_only":  # the whole test passes
            for v in ("eq1_kept", "eq2_lost", "eq0_kept"):
                assert got[v] == [1, 0, 4, 1, 0, 0, 0, 0], msg["name"]
        elif fam == "survivor":  # m = 1: the whole test alone
            for v in ("eq1_kept", "eq2_lost", "eq0_kept"):
                assert got[v] == [1, 0, 1, 1, 0, 0, 0, 0], msg["name"]
        elif fam == "two_survivors":  # m = 2: a whole test and one bit group
            assert got["eq1_kept"] == got["eq2_kept"] == [1, 0, 2, 1, 0, 0, 0, 0], msg["name"]
            assert got["eq0_kept"] == [1, 0, 2, 0, 2, 1, 0, 0]
        else:  # all erroneous, passing chunks, chunks below gt_min, non-batchable requests
            assert all(c == [0] * 8 for c in got.values()), msg["name"]


@pytest.mark.parametrize("eq", [0, 1, 2])
@pytest.mark.parametrize("kept", [0, 1])
def test_model_pass_a_is_the_planners(lists, hostsim, eq, kept):
    """every group-tested chunk of both lists through plan_group_tests_a, the modelled
    results through group_decode"""
    hostsim.hs_group_decode.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    rng = random.Random(5)
    beg, ch, checked = 3, 7, 0  # three directly verified requests first; the chunk's number
    for msg in lists["sweep"] + lists["structure"]:
        for pos, st in R.message_chunks(msg):
            if all(s == 1 for s in st) or len(st) < R.GT_MIN:
                continue
            mc = R.model_chunk(st, eq, bool(kept), rng)
            verdict = [1, 0, -2] + [2 if s != R.ERR else -R.CODE_BAD_ENCODING for s in st]
            # (verify_groups passes chunk_fe = the value was kept and $BLS_GROUP_EQ is not 2)
            off, members, ref, cs, ok = _call(hostsim.hs_plan_group_tests_a, _u32([beg, beg + len(st), ch]), 1,
                                              _i32(verdict), int(eq != 0), int(bool(kept) and eq != 2))
            what = (R.describe(msg), eq, kept)
            if mc is None:
                assert cs == [] and ref == [] and members == [], what
                continue
            checked += 1
            mine = [beg + k for k in mc["ok"]]
            assert ok == mine, what
            first, nbits, whole, has_err, n_ok = cs
            assert (first, nbits, whole, n_ok) == (0, mc["nbits"], int(mc["whole"]), mc["m"]), what
            assert has_err == int(len(mine) < len(st))
            tests = [members[off[g]: off[g + 1]] for g in range(len(ref))]
            assert len(tests) == mc["tests_a"], what
            if whole:
                assert tests[0] == mine and ref[0] == NONE, what
            assert tests[whole:] == [[mine[k] for k in g] for g in mc["groups"]], what
            if eq:
                assert ref[whole:] == [(REF_CHUNK | ch) if mc["from_check"] else first] * nbits, what
                assert not (mc["from_check"] and mc["whole_pass"])  # the chunk check failed
                res = _i32(mc["results"])
                got = hostsim.hs_group_decode(mc["m"], nbits, int(mc["whole_pass"]), ctypes.addressof(res))
                assert got == mc["bad"], what
                assert (got >= 0) == (mc["decided"] == "A")
            else:
                assert not mc["from_check"]
    assert checked == sum(1 for m in lists["sweep"] + lists["structure"]
                          if m["family"] not in ("valid", "small", "nonbatch", "all_err"))
