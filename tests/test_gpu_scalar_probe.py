"""The batch scalars pinned on cuda:0 with cancelling-forgery probes.

Batch verification is sound only if every kernel multiplies set i by r_i = a_i + b_i mu
(bls/pipeline.hpp set_scalar, bls/curve.hpp glv_split).  Valid sets, and sets wrong by a
fixed point, only notice a scalar that differs between the key side and the signature side
of ONE set; a scalar that is consistently wrong (entropy lost, the wrong index hashed, two
sets sharing one) keeps every such test green.  A probe is a batch that is invalid set by
set but whose batch equation holds exactly when the device applies rho_a : rho_b at positions
a and b (tests/_scalarprobe.py; proved against the oracle in tests/test_scalarprobe_cpu.py):

  signature side   sig_a' = sig_a + [rho_b]D, sig_b' = sig_b - [rho_a]D   (any roots; on one
                   shared root by secret keys alone)
  key side         K_a' = [sk_a + rho_b e]g1, K_b' = [sk_b - rho_a e]g1, a and b on one root

with rho computed from the fixed seed by hashlib and integers.  Every probe has a control:
the same construction with one bit (0, 31, 32 or 63, by the case) of r_b flipped before
rho_b is formed, which must be rejected.  Expectations are exact -- verdict lists,
batch_retries, batch_sigs_success, merged_check -- from the scope model of
_scalarprobe.expected_call: a pair cancels exactly when one check covers both members.

The module has its own GpuContext and key table (interop keys 0..15, then the edited keys of
the key-side probes, appended as the cases need them) and runs every call with
DEBUG_MERGED_EVERY_PASS, so the adaptive skip an earlier failing pass leaves on a context
cannot change the expectations.

Not covered, and not faked: set_scalar's r = 0 -> 1 replacement cannot be reached through a
seed (it needs a SHA-256 output with 64 leading zero bits)."""
from __future__ import annotations

import functools
import hashlib

import pytest

from lodestar_amd._abi import (
    DEBUG_FORCE_EXACT,
    DEBUG_GROUP_TEST,
    DEBUG_MERGED_EVERY_PASS,
    DEBUG_MSM,
    DEBUG_NO_MERGED_CHECK,
    DEBUG_NO_MSG_DEDUP,
    DEBUG_NO_PK_COMB,
    DEBUG_NO_UNITS,
    DEBUG_SIGAGG_OFF,
    DEBUG_SIGAGG_ON,
    SSZ_DEPOSIT_MESSAGE,
)
from lodestar_amd.deposits import deposit_domain
from lodestar_amd.native import pack_deposits, pack_requests
from oracle import bls_oracle as O
from tests import _scalarprobe as sp

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
N_KEYS = 16
BITS = (0, 31, 32, 63)
EPS, DELTA = 0x7654321, 0x1234567
PATHS = {
    "pset": DEBUG_SIGAGG_OFF,                           # k_pre's RP / RG lanes + k_pset
    "sigagg": DEBUG_SIGAGG_ON,                          # k_chain roles 2 and 3
    "exact": DEBUG_FORCE_EXACT,                         # stage_exact_set
    "pset_nocomb": DEBUG_SIGAGG_OFF | DEBUG_NO_PK_COMB,
    "sigagg_nocomb": DEBUG_SIGAGG_ON | DEBUG_NO_PK_COMB,
    "exact_nocomb": DEBUG_FORCE_EXACT | DEBUG_NO_PK_COMB,
}
TWO_PATHS = ("pset", "sigagg")
KEYFORMS = ("table", "agg2", "raw96")   # comb rows / the GLV chain on an aggregate / no table


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


@functools.lru_cache(maxsize=None)
def _isk(i: int) -> int:
    return O.interop_secret_key(i)


def _bit(*case) -> int:
    """the control's flipped bit, chosen by the case"""
    return BITS[_h(repr(case).encode())[0] % 4]


class _Probe:
    """the module's context, its growing table and signatures made on the device"""

    def __init__(self, golden):
        from lodestar_amd.native import GpuContext

        self.ctx = GpuContext(0)
        keys = [bytes.fromhex(h) for h in golden["kat2_interop_pubkeys"][:N_KEYS]]
        assert keys == [sp.pk48(_isk(i)) for i in range(N_KEYS)]
        codes = self.ctx.load_pubkeys(b"".join(keys), 48)
        assert list(codes) == [0] * N_KEYS
        self.index = {_isk(i): i for i in range(N_KEYS)}
        self._signed = {}

    def key_index(self, sk: int) -> int:
        """the table index of [sk]g1, appended on first use"""
        if sk not in self.index:
            codes = self.ctx.load_pubkeys(sp.pk48(sk), 48)
            assert list(codes) == [0]
            self.index[sk] = len(self.index)
        return self.index[sk]

    def sign(self, sks, msgs) -> list[bytes]:
        todo = [(s, m) for s, m in dict.fromkeys(zip(sks, msgs)) if (s, m) not in self._signed]
        if todo:
            out = self.ctx.sign(b"".join(s.to_bytes(32, "big") for s, _ in todo), b"".join(m for _, m in todo))
            for k, o in zip(todo, out):
                self._signed[k] = o.tobytes()
        return [self._signed[k] for k in zip(sks, msgs)]

    # -- sets -----------------------------------------------------------------
    def keyref(self, keyform: str, i: int, first_sk: int | None = None):
        """(key reference of set i for pack_requests, the set's secret key); first_sk: the
        set's (first) key replaced by [first_sk]g1"""
        k1 = _isk(i % N_KEYS) if first_sk is None else first_sk
        if keyform == "raw96":
            return sp.pk96(k1), k1
        if keyform == "table":
            return [self.key_index(k1)], k1
        k2 = (i + 5) % N_KEYS
        return [self.key_index(k1), k2], (k1 + _isk(k2)) % sp.R

    def probe(self, kind: str, n: int, a: int, b: int, keyform: str = "table", seed: bytes = SEED, bit=None,
              base: int = 0, tag: bytes = b""):
        """n sets (key i % 16, or that key and key (i + 5) % 16) holding one pair at a and b;
        set i draws its scalar from index base + i.  kind "sig": distinct roots, the general
        signature-side pair; "key": a and b share a root, the key-side pair; "valid": none"""
        tag = tag + kind.encode()
        msgs = [_h(tag + b" root %d" % i) for i in range(n)]
        if kind == "key":
            msgs[b] = msgs[a]
        refs = [self.keyref(keyform, i) for i in range(n)]
        sigs = self.sign([sk for _, sk in refs], msgs)
        keys = [k for k, _ in refs]
        ra, rb = sp.rho(seed, base + a), sp.rho(seed, base + b, bit)
        if kind == "sig":
            sigs[a], sigs[b] = sp.cancelling_sigs(sigs[a], sigs[b], ra, rb)
        elif kind == "key":
            ka, kb = sp.cancelling_sks(_isk(a % N_KEYS), _isk(b % N_KEYS), ra, rb, EPS)
            keys[a], keys[b] = self.keyref(keyform, a, ka)[0], self.keyref(keyform, b, kb)[0]
        return list(zip(keys, msgs, sigs))

    def run(self, reqs, flags: int = 0, seed: bytes = SEED):
        try:
            self.ctx.set_debug_flags(flags | DEBUG_MERGED_EVERY_PASS)
            v, st = self.ctx.verify_packed(pack_requests(reqs, seed=seed))
        finally:
            self.ctx.set_debug_flags(0)
        return [int(x) for x in v], st

    def check(self, reqs, flags, want, where, seed: bytes = SEED):
        """one call against expected_call's (verdicts, retries, sigs_success, merged_check)"""
        v, st = self.run(reqs, flags, seed)
        got = (v, st.batch_retries, st.batch_sigs_success, st.merged_check)
        assert got == tuple(want), "%s: got %s, want %s" % (where, got, tuple(want))
        return st


@pytest.fixture(scope="module")
def pr(golden):
    p = _Probe(golden)
    yield p
    p.ctx.close()


def _one(sets):
    return [(True, [s]) for s in sets]


def _model(n, pairs=(), invalid=(), merged=True):
    return sp.expected_call([[i] for i in range(n)], [True] * n, pairs, invalid, merged)


# ---------------------------------------------------------------------------
# 1. every path that applies a scalar: a and b in one chunk
# ---------------------------------------------------------------------------
_KINDS = {"sig": ("sig", 0), "key_shared_unit": ("key", 0), "key_own_loops": ("key", DEBUG_NO_UNITS | DEBUG_NO_MSG_DEDUP)}


@pytest.mark.parametrize("kind", list(_KINDS))
@pytest.mark.parametrize("keyform", KEYFORMS)
@pytest.mark.parametrize("path", list(PATHS))
def test_pair_in_one_chunk(pr, path, keyform, kind):
    """20 one-set batchable requests, one chunk, the pair at 3 and 17: the probe passes the
    chunk check (all 1, no retry), the control fails it and the fallback rejects a and b.
    The key-side pair runs through the shared Miller-loop unit of its root (sum r_i pk_i)
    and, with DEBUG_NO_UNITS | DEBUG_NO_MSG_DEDUP, through the sets' own loops."""
    n, a, b = 20, 3, 17
    build, extra = _KINDS[kind]
    flags = PATHS[path] | extra
    where = "%s, %s keys, %s" % (path, keyform, kind)
    pr.check(_one(pr.probe(build, n, a, b, keyform)), flags, _model(n, [sp.Pair(a, b)]), where + ", probe")
    bit = _bit(path, keyform, kind)
    want = _model(n, [sp.Pair(a, b, False)])
    assert want == ([0 if i in (a, b) else 1 for i in range(n)], 1, 0, 0)
    pr.check(_one(pr.probe(build, n, a, b, keyform, bit=bit)), flags, want, "%s, control bit %d" % (where, bit))


# ---------------------------------------------------------------------------
# 2. scopes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", TWO_PATHS)
def test_pair_across_chunks(pr, path):
    """32 requests, two chunks of 16, a in chunk 0 and b in chunk 1: the merged check covers
    both (all 1, merged_check 1); with DEBUG_NO_MERGED_CHECK each chunk fails on its own
    member and the fallback rejects a and b; the control fails the merged check too."""
    n, a, b = 32, 3, 20
    probe = _one(pr.probe("sig", n, a, b))
    pr.check(probe, PATHS[path], _model(n, [sp.Pair(a, b)]), path + ", merged")
    want = _model(n, [sp.Pair(a, b)], merged=False)
    assert want == ([0 if i in (a, b) else 1 for i in range(n)], 2, 0, 0)
    pr.check(probe, PATHS[path] | DEBUG_NO_MERGED_CHECK, want, path + ", chunks only")
    bit = _bit(path, "across")
    want = _model(n, [sp.Pair(a, b, False)])
    assert want[1:] == (2, 0, 2)
    pr.check(_one(pr.probe("sig", n, a, b, bit=bit)), PATHS[path], want, "%s, control bit %d" % (path, bit))


@pytest.mark.parametrize("kind", ["sig", "key"])
@pytest.mark.parametrize("path", TWO_PATHS)
def test_chunk_check_after_failed_merged_check(pr, path, kind):
    """The pair in chunk 0, one plainly invalid set (wrong root) in chunk 1: the merged check
    fails, chunk 0 passes on its rebuilt sum, only the invalid set is rejected."""
    n, a, b, bad = 32, 3, 9, 25
    sets = pr.probe(kind, n, a, b)
    sets[bad] = (sets[bad][0], _h(b"not the signed root"), sets[bad][2])
    want = _model(n, [sp.Pair(a, b)], invalid=[bad])
    assert want == ([0 if i == bad else 1 for i in range(n)], 1, 16, 2)
    pr.check(_one(sets), PATHS[path], want, "%s, %s" % (path, kind))
    bit = _bit(path, kind, "after-merged")
    sets = pr.probe(kind, n, a, b, bit=bit)
    sets[bad] = (sets[bad][0], _h(b"not the signed root"), sets[bad][2])
    want = _model(n, [sp.Pair(a, b, False)], invalid=[bad])
    assert want == ([0 if i in (a, b, bad) else 1 for i in range(n)], 2, 0, 2)
    pr.check(_one(sets), PATHS[path], want, "%s, %s, control bit %d" % (path, kind, bit))


@pytest.mark.parametrize("path", TWO_PATHS)
def test_pair_inside_a_non_batchable_request(pr, path):
    """one non-batchable 5-set request holding the pair, alone in the call: the individual
    pass's product over the request's sets"""
    n, a, b = 5, 1, 3
    for kind in ("sig", "key"):
        want = sp.expected_call([list(range(n))], [False], [sp.Pair(a, b)])
        assert want == ([1], 0, 0, 0)
        pr.check([(False, pr.probe(kind, n, a, b))], PATHS[path], want, "%s, %s" % (path, kind))
        bit = _bit(path, kind, "nonbatch")
        want = sp.expected_call([list(range(n))], [False], [sp.Pair(a, b, False)])
        pr.check([(False, pr.probe(kind, n, a, b, bit=bit))], PATHS[path], want,
                 "%s, %s, control bit %d" % (path, kind, bit))


@pytest.mark.parametrize("group_test", [0, DEBUG_GROUP_TEST], ids=["default", "group_test"])
@pytest.mark.parametrize("path", TWO_PATHS)
def test_pair_inside_a_request_of_a_failed_chunk(pr, path, group_test):
    """The same pair inside one batchable 3-set request (sets 4, 5, 6) of a chunk of 18
    requests that fails because of a neighbour (set 12, wrong root): the request verified
    alone -- directly or by the group tests -- is still valid."""
    n, a, b, bad = 20, 4, 6, 12
    req_sets = [[i] for i in range(4)] + [[4, 5, 6]] + [[i] for i in range(7, n)]
    for bit in (None, _bit(path, group_test, "retry")):
        sets = pr.probe("sig", n, a, b, bit=bit)
        sets[bad] = (sets[bad][0], _h(b"not the signed root"), sets[bad][2])
        reqs = [(True, [sets[i] for i in idx]) for idx in req_sets]
        want = sp.expected_call(req_sets, [True] * len(req_sets), [sp.Pair(a, b, bit is None)], invalid=[bad])
        rejected = {bad} if bit is None else {bad, a}
        assert want == ([0 if set(idx) & rejected else 1 for idx in req_sets], 1, 0, 0)
        pr.check(reqs, PATHS[path] | group_test, want, "%s, flipped bit %s" % (path, bit))


@pytest.mark.parametrize("path", TWO_PATHS)
def test_verify_many_offsets_the_index(pr, path):
    """bls_gpu_verify_many over messages of 17, 5 and 19 one-set requests: a is set 4 of
    message 0, b set 7 of message 2, whose scalar index is offset by the earlier messages
    (17 + 5 + 7).  One chunk per message, the merged check over the pass: all 1."""
    sizes, a, b = (17, 5, 19), 4, 17 + 5 + 7
    n = sum(sizes)
    bounds = [0, 17, 22]
    for bit in (None, _bit(path, "many")):
        sets = pr.probe("sig", n, a, b, bit=bit)
        pbs = [pack_requests(_one(sets[lo: lo + sz]), seed=SEED) for lo, sz in zip(bounds, sizes)]
        try:
            pr.ctx.set_debug_flags(PATHS[path] | DEBUG_MERGED_EVERY_PASS)
            vs, st = pr.ctx.verify_many(pbs)
        finally:
            pr.ctx.set_debug_flags(0)
        want = sp.expected_call([[i] for i in range(n)], [True] * n, [sp.Pair(a, b, bit is None)], bounds=bounds)
        assert want[1:] == ((0, n, 1) if bit is None else (2, 5, 2))
        got = ([int(x) for v in vs for x in v], st.batch_retries, st.batch_sigs_success, st.merged_check)
        assert got == want, "%s, flipped bit %s: got %s, want %s" % (path, bit, got, want)


# ---------------------------------------------------------------------------
# 3. bls_gpu_partial: the shards of one call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 0x000000F8, 0x0000FFF8, 0x01020300], ids=lambda v: "base_%#x" % v)
@pytest.mark.parametrize("path", TWO_PATHS)
def test_partial_shards_share_the_index_space(pr, path, base):
    """Two shards of 10 sets, a in shard 0 and b in shard 1 (set_index_base = base and base +
    10): the product of the partials passes, each partial alone fails, and shard 1 made
    with a wrong base breaks the product.  The bases put a carry into every byte of the
    hashed index between a's and b's."""
    n, a, b, half = 20, 3, 13, 10
    sets = pr.probe("sig", n, a, b, base=base)

    def partial(lo, index_base):
        p, status, _, _ = pr.ctx.partial(pack_requests([(True, sets[lo: lo + half])], seed=SEED), index_base)
        assert status == 0
        return p

    try:
        pr.ctx.set_debug_flags(PATHS[path])
        p0, p1 = partial(0, base), partial(half, base + half)
        wrong = [partial(half, wb) for wb in (base + half + 1, (base + half) ^ 0x100, (base + half) ^ 0x01000000)]
        got = [pr.ctx.final_check(ps) for ps in ([p0, p1], [p1, p0], [p0], [p1])]
        got_wrong = [pr.ctx.final_check([p0, w]) for w in wrong]
    finally:
        pr.ctx.set_debug_flags(0)
    assert got == [True, True, False, False], "%s, base %#x: %s" % (path, base, got)
    assert got_wrong == [False] * 3, "%s, base %#x, shard 1 with a wrong base: %s" % (path, base, got_wrong)


# ---------------------------------------------------------------------------
# 4. same-message jobs and deposits
# ---------------------------------------------------------------------------
def test_same_message_job(pr):
    """one job of 10 sets on one root (keys 0..9), the signature-side pair by secret keys at
    2 and 7: all ten verdicts 1; the control's job fails and its sets are told apart"""
    n, a, b = 10, 2, 7
    msg = _h(b"scalarprobe same-message root")
    for bit in (None, _bit("same-message")):
        sks = [_isk(i) for i in range(n)]
        sks[a], sks[b] = sp.cancelling_sks(sks[a], sks[b], sp.rho(SEED, a), sp.rho(SEED, b, bit), DELTA)
        sigs = pr.sign(sks, [msg] * n)
        got, _ = pr.ctx.verify_same_message([(msg, list(range(n)), sigs)], seed=SEED)
        want = [1] * n if bit is None else [0 if i in (a, b) else 1 for i in range(n)]
        assert [int(x) for x in got[0]] == want, "flipped bit %s: %s" % (bit, list(got[0]))


def test_deposits(pr):
    """one bls_gpu_verify_deposits call of 6 deposits; deposits 1 and 4 carry the same key,
    credentials and amount -- one shared DepositMessage -- and the signature-side pair by
    secret keys"""
    n, a, b = 6, 1, 4
    domain = deposit_domain(bytes.fromhex("00000001"))
    owner = [0, 1, 2, 3, 1, 5]
    fields = [(sp.pk48(_isk(k)), _h(b"scalarprobe wc %d" % k), 32 * 10**9 + k) for k in owner]
    objs = b"".join(pk + wc + amount.to_bytes(8, "little") for pk, wc, amount in fields)
    roots = [r.tobytes() for r in pr.ctx.ssz_roots(SSZ_DEPOSIT_MESSAGE, objs, domain)]
    assert roots[a] == roots[b] and len(set(roots)) == n - 1
    for bit in (None, _bit("deposits")):
        sks = [_isk(k) for k in owner]
        sks[a], sks[b] = sp.cancelling_sks(sks[a], sks[b], sp.rho(SEED, a), sp.rho(SEED, b, bit), DELTA)
        sigs = pr.sign(sks, roots)
        rc, v, st = pr.ctx.verify_deposits_packed(
            pack_deposits([f + (s,) for f, s in zip(fields, sigs)], domain, SEED))
        assert rc == 0
        want = _model(n, [sp.Pair(a, b, bit is None)])
        got = ([int(x) for x in v], st.batch_retries, st.batch_sigs_success, st.merged_check)
        assert got == want, "flipped bit %s: got %s, want %s" % (bit, got, want)


# ---------------------------------------------------------------------------
# 5. the Pippenger sum
# ---------------------------------------------------------------------------
def test_msm_sum_across_two_chunks(pr):
    """DEBUG_MSM | DEBUG_SIGAGG_ON at the smallest call whose plan takes k_msm: the merged
    signature sum needs the merged check and more than one chunk (bls_gpu.hip plan_pass:
    use_total), that is 32 one-set requests.  a in chunk 0, b in chunk 1: the probe passes
    the merged check on the MSM's sum of the split scalars, the control fails it."""
    n, a, b = 32, 5, 27
    flags = DEBUG_MSM | DEBUG_SIGAGG_ON
    st = pr.check(_one(pr.probe("sig", n, a, b)), flags, _model(n, [sp.Pair(a, b)]), "k_msm, probe")
    assert st.pass_shape & 1 == 1, "the pass did not take k_msm"
    for bit in BITS:
        want = _model(n, [sp.Pair(a, b, False)])
        assert want == ([0 if i in (a, b) else 1 for i in range(n)], 2, 0, 2)
        st = pr.check(_one(pr.probe("sig", n, a, b, bit=bit)), flags, want, "k_msm, control bit %d" % bit)
        assert st.pass_shape & 1 == 1


# ---------------------------------------------------------------------------
# 6. scalar shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sig", "key"])
@pytest.mark.parametrize("path", TWO_PATHS)
@pytest.mark.parametrize("shape", list(sp.SHAPES))
def test_scalar_shapes(pr, shape, path, kind):
    """A seed under which the scalar at a's index has its top joint 2-bit window zero / a
    zero leading comb digit in both halves / a < 2^16 / b < 2^16: the skipped-addition and
    accumulator-still-infinity branches of jac_mul_glv ([r] sig on G2, [r] pk without rows)
    and g1_comb_mul ([r] pk and [r] g1 on rows, comb on).  a's scalar multiplies b's edit,
    and a's own key and signature."""
    n, a, b = 20, 3, 17
    seed = sp.shape_seed(shape, a)
    assert sp.SHAPES[shape](*sp.halves(sp.r64(seed, a)))
    where = "%s, %s, %s" % (shape, path, kind)
    pr.check(_one(pr.probe(kind, n, a, b, seed=seed)), PATHS[path], _model(n, [sp.Pair(a, b)]), where, seed=seed)
    # the control flips a bit of r_a here (the shaped scalar): the pair with a and b swapped
    bit = _bit(shape, path, kind)
    pr.check(_one(pr.probe(kind, n, b, a, seed=seed, bit=bit)), PATHS[path], _model(n, [sp.Pair(a, b, False)]),
             "%s, control bit %d" % (where, bit), seed=seed)
