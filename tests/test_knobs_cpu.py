"""The BLS_* knobs (lodestar_amd/csrc/bls/knobs.hpp) and the decision table of a verify pass
(plan_pass, bls/plan.hpp), compiled for the CPU (tests/native/plan_exports.hpp in
libhostsim.so).  The parse of every variable, the decisions at their thresholds and the
pass shapes are each checked against a Python restatement of the rule, never against a
second call of the C++.  The same entry points run under -fsanitize=address,undefined in
tests/native/plan_host.cpp (tests/test_plan_cpu.py builds and runs it)."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
OFF = 0xFFFFFFFF
MLF_PAIR = 3
# include/lodestar_bls.h
NO_MSG_DEDUP, NO_MERGED_CHECK, SIGAGG_ON, SIGAGG_OFF, NO_UNITS, DEBUG_MSM, GROUP_TEST = 2, 4, 8, 16, 32, 64, 128
MERGED_EVERY_PASS, MSM_SERIAL = 0x8000, 0x20000


def _atoi(s):
    """C atoi / atol / strtoull(.., 10) on the strings used here (no overflow, no minus for the unsigned)"""
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def _num(unset):
    return lambda e: unset if e is None else _atoi(e)


def _on_unless(v):
    return lambda e: int(not (e is not None and _atoi(e) == v))


def _one_of(allowed):
    return lambda e: _atoi(e) if e is not None and _atoi(e) in allowed else 0


def _gt_min(e):
    x = 4 if e is None else _atoi(e)
    return OFF if x <= 0 else max(x, 2)


# the issue's table: variable -> its value from the variable's text (None: unset)
RULES = {
    "BLS_SIGAGG": lambda e: -1 if e is None or _atoi(e) < 0 else _atoi(e),
    "BLS_PERSET_MAX_INFLIGHT": _num(20480),
    "BLS_DEBUG_SYNC": lambda e: int(e is not None),
    "BLS_GROUP_TEST_MIN": _gt_min,
    "BLS_GROUP_SUMS": _on_unless(0),
    "BLS_GROUP_SUMS_MIN": _num(512),
    "BLS_GROUP_EQ": _num(1),
    "BLS_MSM": lambda e: int(e[0]) if e and e[0] in "01" else -1,
    "BLS_MSM_MIN": _num(60000),
    "BLS_MSM_OVERLAP": _on_unless(0),
    "BLS_ML_SHARED": _on_unless(0),
    "BLS_SIG_TOTAL": _on_unless(0),
    "BLS_MLF_ALONE": _on_unless(0),
    "BLS_MERGED_AFTER_FAIL": _on_unless(1),
    "BLS_SYNC": lambda e: {"spin": 1, "poll": 2}.get(e, 0),
    "BLS_MLF2_WAVES": lambda e: 1 if e is not None and _atoi(e) == 1 else 2,
    "BLS_MLF_PER_LANE": _one_of((1, 2, 4, MLF_PAIR)),
    "BLS_MLF_PAIR_MAX": _num(16384),
    "BLS_MLF_PL2_MIN": _num(98304),
    "BLS_MLF_PL4_MIN": _num(200000),
    "BLS_PACK": _one_of((1, 2, 3)),
    "BLS_PACK_MIN": _num(512),
    "BLS_PACK3_INFLIGHT": _num(2048),
    "BLS_COOP_ML_MAX": _num(8192),
    "BLS_INDIV2_MAX": _num(64),
    "BLS_FE_SIMT_MIN": _num(0),
}
NUMBERS = ["", "0", "1", "7", "123456", "x"]
EDGES = {name: NUMBERS for name in RULES}
EDGES.update({
    "BLS_SIGAGG": ["", "0", "1", "-1", "x", "2"],
    "BLS_MSM": ["0", "1", "2", "01", "", "10", "x"],
    "BLS_GROUP_TEST_MIN": ["0", "-3", "1", "2", "16", ""],
    "BLS_MERGED_AFTER_FAIL": ["0", "1", "2", ""],
    "BLS_SYNC": ["spin", "poll", "Spin", "", "spin "],
    "BLS_MLF_PER_LANE": ["0", "1", "2", "3", "4", "5", ""],
    "BLS_PACK": ["0", "1", "2", "3", "4", ""],
    "BLS_MLF2_WAVES": ["0", "1", "2", "", "x"],
})


def _env(env):
    return "".join(f"{k}={v}\n" for k, v in (env or {}).items()).encode()


def _table(hostsim):
    buf = ctypes.create_string_buffer(1 << 14)
    assert hostsim.hs_knob_table(buf, len(buf)) > 0
    return [tuple(line.split("\t")) for line in buf.value.decode().splitlines()]


def _parse(hostsim, env):
    out = (ctypes.c_uint32 * 256)()
    words = hostsim.hs_knobs_parse(_env(env), out, 256)
    names = [name for name, _ in _table(hostsim)]
    assert words == 1 + 2 * len(names) and out[0] == 2 * len(names)
    vals = {}
    for k, name in enumerate(names):
        v = out[1 + 2 * k] | (out[2 + 2 * k] << 32)
        vals[name] = v - (1 << 64) if v >> 63 else v
    return vals


def test_the_table_is_the_issues(hostsim):
    table = _table(hostsim)
    assert sorted(name for name, _ in table) == sorted(RULES) and len(table) == len(RULES)
    assert all(doc.strip() for _, doc in table)


def test_every_knob_unset(hostsim):
    assert _parse(hostsim, {}) == {name: rule(None) for name, rule in RULES.items()}


@pytest.mark.parametrize("name", sorted(RULES))
def test_knob_parse_edges(hostsim, name):
    for text in EDGES[name]:
        want = {other: rule(None) for other, rule in RULES.items()}
        want[name] = RULES[name](text)
        assert _parse(hostsim, {name: text}) == want, (name, text)


def test_knob_parse_reads_each_variable_from_its_own_name(hostsim):
    """every variable set at once, each to another number: no field takes a neighbour's text"""
    env = {name: str(k + 2) for k, name in enumerate(sorted(RULES))}
    assert _parse(hostsim, env) == {name: RULES[name](env[name]) for name in RULES}


def test_knob_names_are_documented(hostsim):
    """INTEGRATION.md's knob table carries every variable of the table"""
    doc = (ROOT / "INTEGRATION.md").read_text()
    missing = [name for name, _ in _table(hostsim) if f"`{name}`" not in doc]
    assert not missing, missing


# ---- the decisions at their thresholds -------------------------------------------------------

def _decide(hostsim, which, env=None, flags=0, n=0, in_flight=0):
    hostsim.hs_knob_decide.restype = ctypes.c_ulonglong
    return hostsim.hs_knob_decide(_env(env), which, ctypes.c_uint32(flags), ctypes.c_uint32(n),
                                  ctypes.c_ulonglong(in_flight))


def test_use_sigagg(hostsim):
    def sigagg(n, in_flight, env=None, flags=0):
        return _decide(hostsim, 0, env, flags, n, in_flight)

    for in_flight in (0, 20480, 20481, 10 ** 6):
        for n in (1, 511, 512, 2048, 2049, 4096):
            # from 512 sets on, unless the call has at most 2,048 and the process at most 20,480 in flight
            want = n >= 512 and (n > 2048 or in_flight > 20480)
            assert sigagg(n, in_flight) == int(want), (n, in_flight)
            assert sigagg(n, in_flight, flags=SIGAGG_ON) == 1 and sigagg(n, in_flight, flags=SIGAGG_OFF) == 0
            assert sigagg(n, in_flight, flags=SIGAGG_ON | SIGAGG_OFF) == 1  # _ON is looked at first
            assert sigagg(n, in_flight, {"BLS_SIGAGG": "1"}) == 1 and sigagg(n, in_flight, {"BLS_SIGAGG": "0"}) == 0
            assert sigagg(n, in_flight, {"BLS_SIGAGG": "-1"}) == int(want)
            # a debug flag wins over the variable
            assert sigagg(n, in_flight, {"BLS_SIGAGG": "1"}, SIGAGG_OFF) == 0
            assert sigagg(n, in_flight, {"BLS_SIGAGG": "0"}, SIGAGG_ON) == 1
    assert sigagg(1024, 100, {"BLS_PERSET_MAX_INFLIGHT": "100"}) == 0
    assert sigagg(1024, 101, {"BLS_PERSET_MAX_INFLIGHT": "100"}) == 1


def test_msm_on(hostsim):
    assert [_decide(hostsim, 1, in_flight=k) for k in (0, 60000, 60001)] == [0, 0, 1]
    assert [_decide(hostsim, 1, {"BLS_MSM_MIN": "10"}, in_flight=k) for k in (10, 11)] == [0, 1]
    for k in (0, 60001):
        assert _decide(hostsim, 1, {"BLS_MSM": "1"}, in_flight=k) == 1
        assert _decide(hostsim, 1, {"BLS_MSM": "0"}, in_flight=k) == 0
        assert _decide(hostsim, 1, {"BLS_MSM": "2"}, in_flight=k) == int(k > 60000)


def test_group_test_and_group_sums_min(hostsim):
    assert _decide(hostsim, 2) == 4 and _decide(hostsim, 2, flags=GROUP_TEST) == 4
    assert _decide(hostsim, 2, {"BLS_GROUP_TEST_MIN": "0"}) == OFF
    assert _decide(hostsim, 2, {"BLS_GROUP_TEST_MIN": "0"}, GROUP_TEST) == 4
    assert _decide(hostsim, 2, {"BLS_GROUP_TEST_MIN": "16"}) == 16
    assert _decide(hostsim, 2, {"BLS_GROUP_TEST_MIN": "16"}, GROUP_TEST) == 4
    size_max = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1
    assert _decide(hostsim, 3) == 512
    assert _decide(hostsim, 3, {"BLS_GROUP_SUMS_MIN": "0"}) == 0
    assert _decide(hostsim, 3, {"BLS_GROUP_SUMS": "0"}) == size_max
    assert _decide(hostsim, 3, {"BLS_GROUP_SUMS": "0", "BLS_GROUP_SUMS_MIN": "7"}) == size_max
    assert _decide(hostsim, 3, {"BLS_GROUP_SUMS": "1", "BLS_GROUP_SUMS_MIN": "7"}) == 7


def test_wait_blocks(hostsim):
    for n in (0, 2048, 2049, 1 << 20):
        assert _decide(hostsim, 4, n=n) == int(n > 2048)
        assert _decide(hostsim, 4, {"BLS_SYNC": "spin"}, n=n) == 0
        assert _decide(hostsim, 4, {"BLS_SYNC": "poll"}, n=n) == 1
        assert _decide(hostsim, 4, {"BLS_SYNC": "Spin"}, n=n) == int(n > 2048)


def test_mlf_per_lane(hostsim):
    want = {0: MLF_PAIR, 16384: MLF_PAIR, 16385: 1, 98304: 1, 98305: 2, 200000: 2, 200001: 4}
    for in_flight, pl in want.items():
        assert _decide(hostsim, 5, in_flight=in_flight) == pl, in_flight
        for fixed in (1, 2, 3, 4):
            assert _decide(hostsim, 5, {"BLS_MLF_PER_LANE": str(fixed)}, in_flight=in_flight) == fixed
        assert _decide(hostsim, 5, {"BLS_MLF_PER_LANE": "5"}, in_flight=in_flight) == pl
    env = {"BLS_MLF_PAIR_MAX": "10", "BLS_MLF_PL2_MIN": "20", "BLS_MLF_PL4_MIN": "30"}
    assert [_decide(hostsim, 5, env, in_flight=k) for k in (10, 11, 20, 21, 30, 31)] == [MLF_PAIR, 1, 1, 2, 2, 4]


def test_mlf_per_lane_alone(hostsim):
    assert [_decide(hostsim, 6, n=c) for c in (1, 16384, 16385)] == [MLF_PAIR, MLF_PAIR, 1]
    assert [_decide(hostsim, 6, {"BLS_MLF_PAIR_MAX": "10"}, n=c) for c in (10, 11)] == [MLF_PAIR, 1]
    for c in (1, 16384, 16385):
        assert _decide(hostsim, 6, {"BLS_MLF_ALONE": "0"}, n=c) == 0
        assert _decide(hostsim, 6, {"BLS_MLF_ALONE": "0", "BLS_MLF_PER_LANE": "2"}, n=c) == 0  # off wins
        for fixed in (1, 2, 3, 4):
            assert _decide(hostsim, 6, {"BLS_MLF_PER_LANE": str(fixed)}, n=c) == fixed


def test_pack_for(hostsim):
    for n in (1, 511, 512, 4096):
        for in_flight in (0, 2048, 2049):
            want = 1 if n < 512 else (3 if in_flight > 2048 else 2)
            assert _decide(hostsim, 7, n=n, in_flight=in_flight) == want, (n, in_flight)
            for forced in (1, 2, 3):
                assert _decide(hostsim, 7, {"BLS_PACK": str(forced)}, n=n, in_flight=in_flight) == forced
            assert _decide(hostsim, 7, {"BLS_PACK": "4"}, n=n, in_flight=in_flight) == want
    assert [_decide(hostsim, 7, {"BLS_PACK_MIN": "100"}, n=n) for n in (99, 100)] == [1, 2]
    assert [_decide(hostsim, 7, {"BLS_PACK3_INFLIGHT": "5"}, n=600, in_flight=k) for k in (5, 6)] == [2, 3]


# ---- plan_pass ---------------------------------------------------------------------------------

SHAPE = ("n R n_chunks n_uniq n_pk_idx partial sm dedup dep merged_eligible merged_skipped merged sigagg use_units "
         "smsum use_total use_msm msm_overlap ml_shared n_units unit_base indiv_vbase n_total n_prod gt_min gt_possible "
         "gt_eq_mode gsums_min fe_min fe_simt_possible init_set_flag pack mlf_pl pl_forced merged_after_fail gseg_cap "
         "gtmp_cap grp_cap grp_mem_cap").split()
SIZES = "chunk_gsum unit_gsum total_gsum total_levels ml_dom agg_list msg_uniq".split()
PLAIN, PARTIAL, DEPOSIT, SAME_MSG = range(4)


def _u32(xs):
    xs = list(xs)
    return (ctypes.c_uint32 * max(1, len(xs)))(*xs)


def _pass(hostsim, R=64, env=None, flags=0, failed=False, in_flight=0, ask=PLAIN, aux=None, batchable=None,
          roots=None, req_sizes=None):
    """plan_pass over R requests (one set each unless req_sizes), all batchable unless
    `batchable`, every set its own root unless `roots` -> the shape, the plans' sizes, chunk_off"""
    req_sizes = [1] * R if req_sizes is None else req_sizes
    req_off = [0]
    for s in req_sizes:
        req_off.append(req_off[-1] + s)
    n = req_off[-1]
    roots = list(range(n)) if roots is None else roots
    batchable = [1] * R if batchable is None else batchable
    out = (ctypes.c_uint32 * 4096)()
    words = hostsim.hs_plan_pass(_env(env), _u32(req_off), R, bytes(batchable) + b"\0", _u32(roots), ask,
                                 _u32(aux) if aux is not None else None, max(0, len(aux or []) - 1),
                                 ctypes.c_uint32(flags), int(failed), ctypes.c_ulonglong(in_flight), out, 4096)
    assert words > 0
    vecs, at = [], 0
    while at < words:
        vecs.append(list(out[at + 1: at + 1 + out[at]]))
        at += 1 + out[at]
    shape, sizes, chunk_off = vecs
    assert len(shape) == len(SHAPE) and len(sizes) == len(SIZES)
    sh = dict(zip(SHAPE, shape), **dict(zip(SIZES, sizes)))
    # what every pass keeps, whatever its shape: the f / chain layout and the workspace caps
    C = len(chunk_off) - 1
    assert sh["n"] == n and sh["R"] == R and sh["n_chunks"] == C
    assert sh["unit_base"] == n + C and sh["indiv_vbase"] == n + C + sh["n_units"]
    assert sh["n_total"] == (sh["indiv_vbase"] + R if sh["sigagg"] else n)
    assert sh["n_prod"] == (sh["indiv_vbase"] if sh["sigagg"] else n)
    assert sh["gseg_cap"] == 2 * (n // 2 + 12 * R + 8) and sh["gtmp_cap"] == n // 4 + R + 1
    assert sh["merged"] == int(sh["merged_eligible"] and not sh["merged_skipped"])
    assert sh["merged_after_fail"] == int(failed and ask != DEPOSIT)
    assert sh["msm_overlap"] <= sh["use_msm"] <= sh["use_total"] <= min(sh["merged"], sh["sigagg"])
    return sh, chunk_off


def _has(sh, **want):
    got = {k: sh[k] for k in want}
    assert got == {k: int(v) for k, v in want.items()}


def test_plan_pass_base_case(hostsim):
    """64 one-set batchable requests, four chunks of 16, the aggregated path forced"""
    sh, chunk_off = _pass(hostsim, flags=SIGAGG_ON)
    assert chunk_off == [0, 16, 32, 48, 64]
    _has(sh, n=64, R=64, n_chunks=4, n_uniq=64, n_pk_idx=64, partial=0, sm=0, dedup=0, dep=0, merged_eligible=1,
         merged_skipped=0, merged=1, sigagg=1, use_units=0, smsum=0, use_total=1, use_msm=0, msm_overlap=0,
         ml_shared=1, n_units=0, unit_base=68, indiv_vbase=68, n_total=132, n_prod=68, gt_min=4, gt_possible=1,
         gt_eq_mode=1, gsums_min=512, fe_min=0, fe_simt_possible=0, init_set_flag=0, pack=0, mlf_pl=0, pl_forced=0,
         merged_after_fail=0, grp_cap=64 + 14 * 4 + 2, grp_mem_cap=8 * 64 + 16)
    # the chunk groups' sum plan over every set, the one total group over the same sets, one
    # product domain per item of [0, unit_base)
    _has(sh, chunk_gsum=64, unit_gsum=0, total_gsum=64, ml_dom=68, agg_list=0, msg_uniq=64)
    # without a forced path a 64-set call is the per-set one: no sums, no virtual sets
    sh, _ = _pass(hostsim)
    _has(sh, sigagg=0, merged=1, use_total=0, use_msm=0, ml_shared=0, n_total=64, n_prod=64, chunk_gsum=0, ml_dom=0)
    sh, _ = _pass(hostsim, env={"BLS_SIGAGG": "1"})
    _has(sh, sigagg=1, use_total=1)
    sh, _ = _pass(hostsim, env={"BLS_SIGAGG": "1"}, flags=SIGAGG_OFF)
    _has(sh, sigagg=0)


def test_plan_pass_msm_by_sets_in_flight(hostsim):
    _has(_pass(hostsim, flags=SIGAGG_ON, in_flight=60000)[0], use_total=1, use_msm=0, msm_overlap=0)
    _has(_pass(hostsim, flags=SIGAGG_ON, in_flight=60001)[0], use_total=1, use_msm=1, msm_overlap=1)
    _has(_pass(hostsim, flags=SIGAGG_ON, in_flight=60001, env={"BLS_MSM_OVERLAP": "0"})[0], use_msm=1, msm_overlap=0)
    _has(_pass(hostsim, flags=SIGAGG_ON, in_flight=60001, env={"BLS_MSM": "0"})[0], use_total=1, use_msm=0)
    _has(_pass(hostsim, flags=SIGAGG_ON, in_flight=60001, env={"BLS_SIG_TOTAL": "0"})[0], use_total=0, use_msm=0)
    # the per-set path has no sum to replace
    _has(_pass(hostsim, flags=SIGAGG_OFF, in_flight=60001)[0], use_total=0, use_msm=0)
    # BLS_DEBUG_MSM forces it, _MSM_SERIAL keeps its stages in front of the Miller loops
    _has(_pass(hostsim, flags=SIGAGG_ON | DEBUG_MSM)[0], use_msm=1, msm_overlap=1)
    _has(_pass(hostsim, flags=SIGAGG_ON | DEBUG_MSM | MSM_SERIAL)[0], use_msm=1, msm_overlap=0)
    _has(_pass(hostsim, flags=SIGAGG_ON | DEBUG_MSM, env={"BLS_MSM": "0"})[0], use_msm=1)


def test_plan_pass_after_a_failed_merged_check(hostsim):
    on = dict(flags=SIGAGG_ON, in_flight=60001, failed=True)
    _has(_pass(hostsim, **on)[0], merged_eligible=1, merged_skipped=1, merged=0, use_total=0, use_msm=0, msm_overlap=0)
    # a deposit call neither reads nor writes the history
    sh, _ = _pass(hostsim, ask=DEPOSIT, **on)
    _has(sh, dep=1, merged_skipped=0, merged=1, use_total=1, use_msm=1, n_pk_idx=0, n_uniq=64, dedup=0, msg_uniq=0)
    # the merged check stays on: it sums once, but by the per-set chains (a failing pass needs them)
    for keep in (dict(flags=SIGAGG_ON | MERGED_EVERY_PASS), dict(flags=SIGAGG_ON, env={"BLS_MERGED_AFTER_FAIL": "1"})):
        sh, _ = _pass(hostsim, in_flight=60001, failed=True, **keep)
        _has(sh, merged_skipped=0, merged=1, use_total=1, use_msm=0)
    _has(_pass(hostsim, in_flight=60001, failed=True, flags=SIGAGG_ON, env={"BLS_MERGED_AFTER_FAIL": "2"})[0],
         merged_skipped=1, merged=0)
    # ... unless BLS_DEBUG_MSM forces the Pippenger sum
    _has(_pass(hostsim, failed=True, flags=SIGAGG_ON | MERGED_EVERY_PASS | DEBUG_MSM)[0], use_msm=1)
    # a pass that passed: nothing skipped
    _has(_pass(hostsim, flags=SIGAGG_ON, in_flight=60001)[0], merged_skipped=0, merged=1)


def test_plan_pass_merged_check_eligibility(hostsim):
    _has(_pass(hostsim, flags=SIGAGG_ON, ask=PARTIAL)[0], partial=1, merged_eligible=0, merged=0, use_total=0)
    _has(_pass(hostsim, flags=SIGAGG_ON | NO_MERGED_CHECK)[0], merged_eligible=0, merged=0, use_total=0)
    # one non-batchable request: 63 batchable ones in 3 chunks of 21, no merged check
    sh, chunk_off = _pass(hostsim, flags=SIGAGG_ON, batchable=[1] * 30 + [0] + [1] * 33)
    assert chunk_off == [0, 21, 42, 63]
    _has(sh, n_chunks=3, merged_eligible=0, merged=0, merged_skipped=0, use_total=0, unit_base=67, n_total=67 + 64)
    _has(_pass(hostsim, flags=SIGAGG_ON, batchable=[1] * 30 + [0] + [1] * 33, failed=True)[0], merged_skipped=0)
    # 16 requests are one chunk: nothing to merge (31 too; 32 are two)
    for R, C in ((16, 1), (31, 1), (32, 2)):
        sh, chunk_off = _pass(hostsim, R=R, flags=SIGAGG_ON)
        assert len(chunk_off) - 1 == C
        _has(sh, merged_eligible=C > 1, merged=C > 1, use_total=C > 1)
    # verify_many: chunks never straddle a message -- 40 + 24 requests are 20 + 20 + 24
    sh, chunk_off = _pass(hostsim, flags=SIGAGG_ON, aux=[0, 40, 64])
    assert chunk_off == [0, 20, 40, 64]
    _has(sh, merged=1, use_total=1, n_chunks=3)


def test_plan_pass_without_sets(hostsim):
    sh, chunk_off = _pass(hostsim, R=2, req_sizes=[0, 0], flags=SIGAGG_ON, in_flight=60001)
    assert chunk_off == [0, 2]
    _has(sh, n=0, sigagg=0, merged_eligible=0, merged=0, use_total=0, use_msm=0, ml_shared=0, n_total=0, n_prod=0,
         unit_base=1, indiv_vbase=1, n_uniq=0, dedup=0, gt_possible=0)


def test_plan_pass_same_message(hostsim):
    jobs = [0, 20, 64]  # two jobs of 20 and 44 sets: two caller-defined chunks, whatever their size
    roots = [0] * 20 + [1] * 44
    for flags in (0, SIGAGG_OFF, NO_UNITS):
        for failed in (False, True):
            sh, chunk_off = _pass(hostsim, ask=SAME_MSG, aux=jobs, roots=roots, flags=flags, failed=failed,
                                  in_flight=60001)
            assert chunk_off == jobs
            _has(sh, sm=1, sigagg=1, use_units=1, smsum=1, n_units=2, n_uniq=2, dedup=1, merged_eligible=1,
                 merged_skipped=0, merged=1, use_total=0, use_msm=0, unit_base=66, indiv_vbase=68, n_total=132,
                 n_prod=68, chunk_gsum=0, unit_gsum=0, ml_dom=68)
    # a 1-set job is a request verified on its own: not batchable, so no merged check
    sh, chunk_off = _pass(hostsim, ask=SAME_MSG, aux=[0, 20, 21, 64], roots=[0] * 20 + [1] + [2] * 43)
    assert chunk_off == [0, 20, 63]
    _has(sh, sm=1, sigagg=1, n_units=2, smsum=1, merged_eligible=0, merged=0)


def test_plan_pass_units_of_shared_roots(hostsim):
    roots = [i // 8 for i in range(64)]  # 8 roots, two per chunk of 16: 8 units for 64 loops
    sh, _ = _pass(hostsim, roots=roots, flags=SIGAGG_ON)
    _has(sh, n_uniq=8, dedup=1, use_units=1, smsum=0, n_units=8, unit_base=68, indiv_vbase=76, n_total=140, n_prod=76,
         unit_gsum=64, chunk_gsum=64, ml_dom=76, msg_uniq=8)
    for flags in (SIGAGG_ON | NO_UNITS, SIGAGG_ON | NO_MSG_DEDUP):
        sh, _ = _pass(hostsim, roots=roots, flags=flags)
        _has(sh, use_units=0, n_units=0, indiv_vbase=68, n_total=132, unit_gsum=0, ml_dom=68,
             dedup=not flags & NO_MSG_DEDUP)
    sh, _ = _pass(hostsim, roots=roots, flags=SIGAGG_OFF)  # the per-set path pairs every set itself
    _has(sh, dedup=1, use_units=0, n_units=0, n_total=64, n_prod=64)
    # units that would not halve the chunks' loops are refused: 9 roots in every chunk of 16
    sh, _ = _pass(hostsim, roots=[(i % 16) % 9 for i in range(64)], flags=SIGAGG_ON)
    _has(sh, dedup=1, use_units=0, n_units=0)


def test_plan_pass_group_tests_possible(hostsim):
    _has(_pass(hostsim, R=3)[0], gt_min=4, gt_possible=0, grp_cap=0, grp_mem_cap=0)
    _has(_pass(hostsim, R=4)[0], gt_min=4, gt_possible=1, grp_cap=4 + 14 + 2, grp_mem_cap=8 * 4 + 16)
    _has(_pass(hostsim, R=3, env={"BLS_GROUP_TEST_MIN": "3"})[0], gt_min=3, gt_possible=1)
    _has(_pass(hostsim, R=64, env={"BLS_GROUP_TEST_MIN": "0"})[0], gt_min=OFF, gt_possible=0, grp_cap=0)
    _has(_pass(hostsim, R=64, env={"BLS_GROUP_TEST_MIN": "17"})[0], gt_min=17, gt_possible=0)
    _has(_pass(hostsim, R=64, env={"BLS_GROUP_TEST_MIN": "17"}, flags=GROUP_TEST)[0], gt_min=4, gt_possible=1)
    # only batchable requests sit in chunks
    _has(_pass(hostsim, R=8, batchable=[1, 1, 1, 0, 0, 0, 0, 0])[0], gt_possible=0)
    sh, _ = _pass(hostsim, env={"BLS_GROUP_EQ": "2", "BLS_GROUP_SUMS": "0", "BLS_FE_SIMT_MIN": "4"})
    _has(sh, gt_eq_mode=2, gsums_min=OFF, fe_min=4, fe_simt_possible=1)
    _has(_pass(hostsim, R=3, env={"BLS_FE_SIMT_MIN": "4"})[0], fe_min=4, fe_simt_possible=0)


def test_plan_pass_debug_shape_flags(hostsim):
    sh, _ = _pass(hostsim, flags=1 | (2 << 8) | (4 << 12))  # _FORCE_EXACT, _PACK(2), _MLF_PL(4)
    _has(sh, init_set_flag=1, pack=2, mlf_pl=4, pl_forced=1)


@pytest.mark.parametrize("flags", [SIGAGG_ON, SIGAGG_OFF])
def test_plan_pass_layout_identities(hostsim, flags):
    """_pass asserts unit_base, indiv_vbase, n_total and n_prod for every shape: here over
    requests of 0 .. 5 sets, shared roots, non-batchable requests and every ask"""
    req_sizes = [(7 * r) % 6 for r in range(70)]
    n = sum(req_sizes)
    roots = [i // 6 for i in range(n)]
    batchable = [int(r % 9 != 4) for r in range(70)]
    for ask in (PLAIN, PARTIAL):
        for failed in (False, True):
            sh, _ = _pass(hostsim, R=70, req_sizes=req_sizes, roots=roots, batchable=batchable, flags=flags, ask=ask,
                          failed=failed, in_flight=10 ** 6)
            assert sh["sigagg"] == int(flags == SIGAGG_ON) and sh["merged_eligible"] == 0
    sh, _ = _pass(hostsim, R=70, req_sizes=req_sizes, roots=roots, flags=flags, in_flight=10 ** 6)
    _has(sh, merged=1, use_total=flags == SIGAGG_ON, use_msm=flags == SIGAGG_ON)
    sh, _ = _pass(hostsim, R=70, flags=flags, ask=DEPOSIT)
    _has(sh, dep=1, merged=1, sigagg=flags == SIGAGG_ON)
