"""The recovery sweep: worker messages whose chunks fail in every way the group tests of a
failed chunk (bls_gpu.hip VerifyPass::verify_groups) index differently, with what each
message must come back as -- verdicts and worker counters from the oracle's worker
semantics (oracle.verify_many_signature_sets over validity tokens), and the eight round
counters of bls_gpu_group_test_counts from a model of the rounds.

The model is written from the comment above group_test_min in bls/knobs.hpp (and the one
on Knobs::group_eq), not from verify_groups: a chunk's requests of status OK are indexed
0 .. m-1, bit group G_j holds those with bit j set, a test passes iff its requests' values
multiply to the identity.  A request's value is modelled additively, as in
test_hostsim.py::test_group_decode_complement_inference: 0 for a valid request, a random
non-zero element of Z_q for an invalid one; a test passes iff its sum is 0.

Only hashlib, integers and the oracle are used here; signatures are attached by
materialize() with whatever signer the caller has (the GPU tests: GpuContext.sign).

Set tokens: 1 valid, 0 invalid (it carries its neighbour's valid signature), ERR erroneous
(a 96-byte zero signature: BAD_ENCODING).
"""
from __future__ import annotations

import hashlib
import itertools
import random

ERR = "E"
CODE_BAD_ENCODING = 1  # BLST_BAD_ENCODING
Q = (1 << 61) - 1  # the additive model of the target group: 0 = identity
N_KEYS = 100  # the interop keys of tests/golden (the device table the GPU tests load)
GT_MIN = 4  # $BLS_GROUP_TEST_MIN's default
SINGLE_M = (4, 5, 8, 9, 16, 17, 31)  # both sides of every nbits step, and the largest single chunk
STRUCT_SETS = (1, 4, 5, 16, 17)  # sets per request: both sides of BLS_FOLD1 = 4 and BLS_FOLD = 16

# the counter variants: (complement-inference mode $BLS_GROUP_EQ, chunk-check value kept, gt_min)
VARIANTS = {
    "eq1_kept": (1, True, GT_MIN), "eq1_lost": (1, False, GT_MIN),
    "eq2_kept": (2, True, GT_MIN), "eq2_lost": (2, False, GT_MIN),
    "eq0_kept": (0, True, GT_MIN), "eq0_lost": (0, False, GT_MIN),
    "gt_off": (1, True, 0), "gt16": (1, True, 16),
}


def chunk_bounds(n, min_per_chunk=16):
    """chunkifyMaximizeChunkSize (multithread/utils.ts:4-19): the chunk bounds of n requests"""
    count = n // min_per_chunk
    if count <= 1:
        return [0, n]
    per = -(-n // count)
    return list(range(0, n, per)) + [n]


def nbits_of(m):
    """ceil(log2 m) bit groups (none for m <= 1)"""
    return (m - 1).bit_length() if m > 1 else 0


def req_status(tokens):
    """a request's outcome: ERR when a signature does not decode, else 1 / 0"""
    if any(t == ERR for t in tokens):
        return ERR
    return 1 if all(t == 1 for t in tokens) else 0


# ---- the model of the rounds ----------------------------------------------------------------

def model_chunk(status, eq, kept, rng):
    """One group-tested chunk: status per request (1, 0, ERR).  Returns None when no request
    is of status OK (nothing is planned), else a dict: m, nbits, whole (a test of all the OK
    requests runs), from_check (the chunk check's value stands for it), groups (the bit
    groups as lists of OK-index positions), whole_pass, results (per bit group: bit 0 passed,
    bit 1 its value equals the whole's), decided ('A', 'B' or 'C'), bad (the position pass
    A named, len(ok) for none, -1 undecided), tests_b, tests_c, and the verdict per OK
    request."""
    ok = [k for k, s in enumerate(status) if s != ERR]
    m = len(ok)
    if m == 0:
        return None
    has_err = m < len(status)
    val = [0 if status[k] == 1 else rng.randrange(1, Q) for k in ok]
    nbits = nbits_of(m)
    groups = [[k for k in range(m) if (k >> j) & 1] for j in range(nbits)]
    gsum = [sum(val[k] for k in g) % Q for g in groups]
    total = sum(val) % Q
    out = {"m": m, "nbits": nbits, "groups": groups, "ok": ok, "tests_b": 0, "tests_c": 0, "bad": -1}
    truth = [1 if v == 0 else 0 for v in val]
    if eq:
        # the whole's value: the failed chunk check's own, usable when it was kept, ran over
        # exactly these requests (none erroneous) and m > 1; else a test of them
        out["from_check"] = eq == 1 and kept and not has_err and m > 1
        out["whole"] = not out["from_check"]
        out["whole_pass"] = total == 0
        out["results"] = [(1 if s == 0 else 0) | (2 if s == total else 0) for s in gsum]
        if total == 0:
            bad = m  # every request valid
        elif m == 1:
            bad = 0
        else:
            # G_j fails iff its sum is not 0; rest_j fails iff total - sum is not 0: one invalid
            # request fails exactly one of the two for every bit, which names it
            bad = 0
            for j, s in enumerate(gsum):
                g_fails, rest_fails = s != 0, (total - s) % Q != 0
                if g_fails == rest_fails:
                    bad = -1
                    break
                if g_fails:
                    bad |= 1 << j
            if bad >= m:
                bad = -1
        out["bad"] = bad
        out["decided"] = "A" if bad >= 0 else "C"
    else:
        # two rounds: a whole test only for a chunk with an erroneous request or a single one
        out["from_check"] = False
        out["whole"] = has_err or m == 1
        out["whole_pass"] = total == 0
        out["results"] = [1 if s == 0 else 0 for s in gsum]
        if out["whole"] and (total == 0 or m == 1):
            out["decided"], out["bad"] = "A", (m if total == 0 else 0)
        else:
            idx = 0
            for j, s in enumerate(gsum):
                if s != 0:
                    idx |= 1 << j
            if idx < m:
                out["tests_b"] = 2  # {idx} alone, the rest together
                rest = (total - val[idx]) % Q
                if val[idx] != 0 and rest == 0:
                    out["decided"], out["bad"] = "B", idx
                else:
                    out["decided"] = "C"
            else:
                out["decided"] = "C"
    if out["decided"] == "C":
        out["tests_c"] = m
        out["verdicts"] = truth  # every request alone
    else:
        out["verdicts"] = [0 if k == out["bad"] else 1 for k in range(m)]
    out["tests_a"] = (1 if out["whole"] else 0) + nbits
    return out


def chunk_counters(mc):
    """the eight counters one modelled chunk adds"""
    c = [0] * 8
    if mc is None:
        return c
    c[0] = 1
    c[1] = 1 if mc["from_check"] else 0
    c[2] = mc["tests_a"]
    c[3] = 1 if mc["decided"] == "A" else 0
    c[4] = mc["tests_b"]
    c[5] = 1 if mc["decided"] == "B" else 0
    c[6] = mc["tests_c"]
    return c


def message_chunks(msg):
    """the statuses of a message's batchable requests, chunk by chunk: (positions, statuses)"""
    idx = [r for r, (b, _) in enumerate(msg["reqs"]) if b]
    st = [req_status(msg["reqs"][r][1]) for r in idx]
    bounds = chunk_bounds(len(idx)) if idx else [0]
    return [(idx[a:b], st[a:b]) for a, b in zip(bounds, bounds[1:])]


def model_message(msg, variant, seed=7):
    """(verdicts, counters) of one message under a counter variant, from the model alone"""
    eq, kept, gt_min = VARIANTS[variant]
    rng = random.Random(hashlib.sha256(b"%d|" % seed + msg["name"].encode()).digest())
    verdicts = [None] * len(msg["reqs"])
    counters = [0] * 8
    for r, (b, toks) in enumerate(msg["reqs"]):
        if not b:
            s = req_status(toks)
            verdicts[r] = -CODE_BAD_ENCODING if s == ERR else s
    for pos, st in message_chunks(msg):
        if all(s == 1 for s in st):
            for r in pos:
                verdicts[r] = 1
            continue
        for r, s in zip(pos, st):  # the retry: every request alone
            verdicts[r] = -CODE_BAD_ENCODING if s == ERR else s
        if gt_min == 0 or len(pos) < gt_min:
            continue
        mc = model_chunk(st, eq, kept, rng)
        counters = [a + b for a, b in zip(counters, chunk_counters(mc))]
        if mc is not None:
            for k, v in zip(mc["ok"], mc["verdicts"]):
                verdicts[pos[k]] = v
    return verdicts, counters


def oracle_message(oracle, msg):
    """(verdicts, batch_retries, batch_sigs_success) from the oracle's worker semantics"""
    def maybe_batch(toks):
        if not toks:
            raise oracle.BlsError(oracle.E_EMPTY_SET)
        if any(t == ERR for t in toks):
            raise oracle.BlsError(CODE_BAD_ENCODING)
        return all(t == 1 for t in toks)

    res, retries, ok = oracle.verify_many_signature_sets([(b, list(t)) for b, t in msg["reqs"]], maybe_batch)
    return [(1 if r[1] else 0) if r[0] == "success" else -r[1].code for r in res], retries, ok


# ---- the messages ---------------------------------------------------------------------------

def _msg(name, family, status, sets_per_req=1, batchable=True, **info):
    """a message of one-chunk shape: status per request (1, 0, ERR)"""
    reqs = []
    for s in status:
        toks = [1] * sets_per_req
        if s != 1:
            toks[0] = s
        reqs.append((batchable, toks))
    return dict(name=name, family=family, reqs=reqs, roots=None, m=len(status),
                bad=[k for k, s in enumerate(status) if s == 0], err=[k for k, s in enumerate(status) if s == ERR],
                **info)


def _status(m, bad=(), err=()):
    return [ERR if k in err else (0 if k in bad else 1) for k in range(m)]


def _neighbours():
    """what sits between the failing messages: passing chunks, chunks below gt_min
    (verified directly), non-batchable requests"""
    def small(n):
        out = [_msg("small%d-valid" % n, "small", _status(n))]
        return out + [_msg("small%d-bad%d" % (n, b), "small", _status(n, bad=[b])) for b in range(n)]

    nonbatch = _msg("nonbatch", "nonbatch", [1, 0], batchable=False)
    return ([_msg("valid4", "valid", _status(4))] + small(1) + [_msg("valid16", "valid", _status(16))] + small(2) +
            [_msg("valid31", "valid", _status(31))] + small(3) + [nonbatch])


def sweep_failing():
    """the failing chunks of the sweep, family by family"""
    out = []
    for m in SINGLE_M:
        out += [_msg("single-m%d-b%d" % (m, b), "single", _status(m, bad=[b])) for b in range(m)]
    for m, pairs in ((5, itertools.combinations(range(5), 2)), (16, itertools.combinations(range(16), 2)),
                     (17, ((a, 16) for a in range(16)))):
        out += [_msg("pair-m%d-%d-%d" % (m, a, b), "pair", _status(m, bad=[a, b])) for a, b in pairs]
    out += [_msg("triple-%d-%d-%d" % t, "triple", _status(16, bad=t)) for t in ((0, 1, 2), (5, 10, 15), (13, 14, 15))]
    out += [_msg("shift-e%d-b%d" % (e, b), "shifted", _status(9, bad=[b], err=[e]))
            for e in range(9) for b in range(9) if b != e]
    out += [_msg("erronly-e%d" % e, "err_only", _status(9, err=[e])) for e in range(9)]
    for s in range(4):
        err = [k for k in range(4) if k != s]
        out.append(_msg("survivor%d-valid" % s, "survivor", _status(4, err=err)))
        out.append(_msg("survivor%d-bad" % s, "survivor", _status(4, bad=[s], err=err)))
    out.append(_msg("allerr", "all_err", _status(4, err=range(4))))
    for s in itertools.combinations(range(5), 2):
        err = [k for k in range(5) if k not in s]
        out += [_msg("two-%d-%d-bad%d" % (s[0], s[1], b), "two_survivors", _status(5, bad=[b], err=err)) for b in s]
    return out


def _interleave(failing, neighbours, every):
    """one neighbour (cycling through them) after every `every` failing messages; a
    repeated neighbour gets a name of its own (its sets sign their own roots)"""
    out, k = [], 0
    for i, msg in enumerate(failing):
        out.append(msg)
        if (i + 1) % every == 0:
            nb = dict(neighbours[k % len(neighbours)])
            nb["name"] = "%s#%d" % (nb["name"], k // len(neighbours))
            out.append(nb)
            k += 1
    return out


def sweep():
    """the sweep list: every failing chunk, a neighbour after every eighth"""
    return _interleave(sweep_failing(), _neighbours(), 8)


def structure():
    """chunks of 16 whose requests hold 1, 4, 5, 16 and 17 sets, the one invalid set first /
    last in its request, the request first / last in the chunk; a chunk's sets sign one of two
    roots (alternating), so the first pass pairs them in units and shared loops.  An
    all-valid chunk sits in the middle."""
    out = []
    for s in STRUCT_SETS:
        for req_pos in (0, 15):
            for set_pos in (0, s - 1):
                msg = _msg("struct-s%d-r%d-i%d" % (s, req_pos, set_pos), "structure", _status(16), sets_per_req=s,
                           set_pos=set_pos)
                msg["reqs"][req_pos][1][set_pos] = 0
                msg["bad"] = [req_pos]
                msg["roots"] = [i % 2 for i in range(16 * s)]
                out.append(msg)
    mid = _msg("struct-valid", "valid", _status(16), sets_per_req=4)
    mid["roots"] = [i % 2 for i in range(64)]
    out.insert(len(out) // 2, mid)
    return out


def batchable_only(msgs):
    """the messages without a non-batchable request (a pass with one runs no merged check)"""
    return [m for m in msgs if all(b for b, _ in m["reqs"])]


def expectations(oracle, msgs):
    """per message: verdicts, retries, ok from the oracle, the counters of every variant
    from the model (whose verdicts must be the oracle's: test_recovery_cpu.py)"""
    out = []
    for msg in msgs:
        v, retries, ok = oracle_message(oracle, msg)
        out.append(dict(verdicts=v, retries=retries, ok=ok,
                        counters={name: model_message(msg, name)[1] for name in VARIANTS}))
    return out


def totals(exp, variant):
    """summed worker counters and round counters of a list of expectations"""
    cnt = [0] * 8
    for e in exp:
        cnt = [a + b for a, b in zip(cnt, e["counters"][variant])]
    return sum(e["retries"] for e in exp), sum(e["ok"] for e in exp), cnt


# ---- signatures -----------------------------------------------------------------------------

def _h(b):
    return hashlib.sha256(b).digest()


def materialize(msgs, sign, tag=b"recovery"):
    """The messages as pack_requests() inputs over the device table's keys 0 .. N_KEYS-1.
    sign(key_indices, roots) -> the valid signatures (96 bytes each).  An invalid set carries
    the valid signature of the next set of the whole list (another key: never valid for
    it), an erroneous one 96 zero bytes."""
    keys, roots, toks = [], [], []
    for msg in msgs:
        i = 0
        for _, sets in msg["reqs"]:
            for t in sets:
                keys.append(len(keys) % N_KEYS)
                which = b"set%d" % i if msg["roots"] is None else b"root%d" % msg["roots"][i]
                roots.append(_h(tag + b"|" + msg["name"].encode() + b"|" + which))
                toks.append(t)
                i += 1
    sigs = sign(keys, roots)
    n = len(keys)
    assert n > 1 and all(keys[i] != keys[(i + 1) % n] for i in range(n))
    out, i = [], 0
    for msg in msgs:
        reqs = []
        for b, sets in msg["reqs"]:
            ss = []
            for t in sets:
                sig = bytes(96) if t == ERR else bytes(sigs[i] if t == 1 else sigs[(i + 1) % n])
                ss.append(([keys[i]], roots[i], sig))
                i += 1
            reqs.append((b, ss))
        out.append(reqs)
    return out


def describe(msg):
    """what a failure names: the message, its chunk size and the bad / erroneous positions"""
    return "%s (m=%d, invalid at %s, erroneous at %s)" % (msg["name"], msg["m"], msg["bad"], msg["err"])
