"""One public-key table per device, shared by its contexts (bls_gpu_share_pubkeys,
bls_gpu_pubkeys_info; bls/pk_table.hpp): contexts that share a table verify as a context
with a private replica does, a load through any of them appends for all of them, and a
call in flight never reads a buffer that another context's load freed or moved.

Shapes: loads of 3, then 70, then 1,100 keys (the first capacity is 1,028: the third load
grows the table); calls of 65 single-key sets with DEBUG_SIGAGG_ON |
DEBUG_MERGED_EVERY_PASS (two wavefronts per role, the second with one lane).

Expected verdicts and worker counters follow tests/test_gpu_pk_comb.py: every set's outcome
is known by construction, and oracle.verify_many_signature_sets turns the outcomes into
per-request results, batch retries and successes."""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import threading
from pathlib import Path

import pytest

from lodestar_amd._abi import DEBUG_MERGED_EVERY_PASS, DEBUG_NO_PK_COMB, DEBUG_SIGAGG_ON
from lodestar_amd.native import GpuContext, NativeError, pack_requests

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
N1, N2, N3 = 3, 70, 1100
N = N1 + N2 + N3
CAP1 = N1 + N1 // 2 + 1024  # the capacity after the first load: 1,028
ENTRY, ROWS = 100, 1440     # bytes per key: the table entry (G1A) and its comb rows
SEED = bytes(range(64, 96))
FLAGS = DEBUG_SIGAGG_ON | DEBUG_MERGED_EVERY_PASS


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def _expected(oracle, outcomes):
    """(verdicts, batch_retries, batch_sigs_success) of one worker message of one-set
    batchable requests with the given set outcomes (1 / 0)"""
    res, retries, ok = oracle.verify_many_signature_sets([(True, [o]) for o in outcomes],
                                                         lambda tokens: all(t == 1 for t in tokens))
    assert all(r[0] == "success" for r in res)
    return [1 if r[1] else 0 for r in res], retries, ok


class World:
    """the keys' secrets and compressed keys; table index i of every table below holds key
    sk_of(i)"""

    def __init__(self, gpu, oracle):
        self.gpu = gpu
        self.sks = [oracle.interop_secret_key(i).to_bytes(32, "big") for i in range(N)]
        self.pks = gpu.sk_to_pk(b"".join(self.sks))

    def blob(self, first, n):
        return self.pks[first: first + n].tobytes()

    def sets(self, keys, tag, sk_of=lambda k: k):
        """one valid single-key set per table index in keys"""
        msgs = [_h(tag + b"%d" % i) for i in range(len(keys))]
        sigs = self.gpu.sign(b"".join(self.sks[sk_of(k)] for k in keys), b"".join(msgs))
        return [([k], m, s.tobytes()) for k, m, s in zip(keys, msgs, sigs)]

    def call65(self, keys, tag, sk_of=lambda k: k):
        """65 sets, set 40 signed for another message: (sets, outcomes, the 64 good sets)"""
        assert len(keys) == 65
        sets = self.sets(keys, tag, sk_of)
        good = sets[:40] + sets[41:]
        sets[40] = (sets[40][0], _h(b"another message"), sets[40][2])
        return sets, [0 if i == 40 else 1 for i in range(65)], good


@pytest.fixture(scope="module")
def world(gpu, oracle):
    return World(gpu, oracle)


def _ctx(flags=FLAGS):
    c = GpuContext(0)
    c.base_debug_flags = flags
    c.set_debug_flags(0)
    return c


def _load(c, blob):
    assert (c.load_pubkeys(blob, 48) == 0).all()


def _pair(world, n=N1 + N2):
    """an owner holding the first n keys (loads of 3 and n - 3) and a peer that shares after
    the loads"""
    owner, peer = _ctx(), _ctx()
    _load(owner, world.blob(0, N1))
    _load(owner, world.blob(N1, n - N1))
    peer.share_pubkeys(owner)
    return owner, peer


def _verify(c, sets):
    v, st = c.verify_packed(pack_requests([(True, [s]) for s in sets], seed=SEED))
    return list(v), st


def _check(oracle, ctxs, sets, outcomes):
    want, retries, ok = _expected(oracle, outcomes)
    for name, c in ctxs:
        v, st = _verify(c, sets)
        assert v == want, name
        assert (st.batch_retries, st.batch_sigs_success) == (retries, ok), name


def _partial(c, good):
    rec, status, _err, _st = c.partial(pack_requests([(True, good)], seed=SEED), 0)
    assert status == 0
    return rec


class Trio:
    """owner and peer on one table, and a third context with a private replica of it"""

    def __init__(self, world):
        self.owner, self.peer = _pair(world)
        self.private = _ctx()
        _load(self.private, world.blob(0, N1))
        _load(self.private, world.blob(N1, N2))
        self.grown = False

    def all(self):
        return [("owner", self.owner), ("peer", self.peer), ("private", self.private)]

    def grow(self, world):
        """the third load, through the peer (and into the replica)"""
        if not self.grown:
            _load(self.peer, world.blob(N1 + N2, N3))
            _load(self.private, world.blob(N1 + N2, N3))
            self.grown = True

    def close(self):
        for _, c in self.all():
            c.close()


@pytest.fixture(scope="module")
def trio(world):
    t = Trio(world)
    yield t
    t.close()


def test_peers_verify_alike(trio, world, oracle):
    """a 65-set call over both loads, one set signed for another message: the oracle's
    verdicts and counters on the owner, the peer and the private replica; without the bad
    set the three bls_gpu_partial records are equal byte for byte"""
    keys = [0, 1, 2] + list(range(N1, N1 + 62))
    sets, outcomes, good = world.call65(keys, b"alike-")
    _check(oracle, trio.all(), sets, outcomes)
    recs = [_partial(c, good) for _, c in trio.all()]
    assert recs[0] == recs[1] == recs[2]
    assert trio.owner.final_check([recs[1]])


def test_a_shared_table_reports_itself_as_one(trio):
    """runs before and after the growth alike: ids, the context count, and device_bytes of
    the current generation counted once"""
    o, p, q = (c.pubkeys_info() for _, c in trio.all())
    assert o == p
    assert o["table_id"] != 0 and q["table_id"] not in (0, o["table_id"])
    assert (o["n_contexts"], q["n_contexts"]) == (2, 1)
    assert o["n_keys"] == o["comb_keys"] == q["n_keys"] == (N if trio.grown else N1 + N2)
    if not trio.grown:
        assert o["capacity"] == CAP1
    for i in (o, q):
        assert i["device_bytes"] == i["capacity"] * (ENTRY + ROWS + 1)


def test_an_append_through_the_peer_grows_the_table_for_everyone(trio, world, oracle):
    """the peer loads 1,100 keys (past the first capacity: a new generation); the owner then
    verifies sets naming keys of all three loads, both report the same n_keys, and a set
    naming index n_keys gets what a private table gives an index past its end"""
    trio.grow(world)
    keys = [0, 2, 3, 72] + list(range(1000, 1057)) + [N - 4, N - 3, N - 2, N - 1]
    sets, outcomes, _ = world.call65(keys, b"grown-")
    _check(oracle, trio.all(), sets, outcomes)
    o, p = trio.owner.pubkeys_info(), trio.peer.pubkeys_info()
    assert o == p and o["n_keys"] == N and o["capacity"] > CAP1
    past = [sets[0], ([N], sets[1][1], sets[1][2])]
    want, _ = _verify(trio.private, past)
    assert want[1] != 1
    for name, c in trio.all()[:2]:
        assert _verify(c, past)[0] == want, name
    # and the aggregate path reads the same table (bls_gpu_aggregate_pubkeys)
    lists = [[0, 72, N - 1], [N]]
    aggs = [c.aggregate_pubkeys(lists) for _, c in trio.all()]
    for a, codes in aggs[:2]:
        assert a[0] == aggs[2][0][0] and list(codes) == list(aggs[2][1])
    assert aggs[2][1][0] == 0 and aggs[2][1][1] != 0


def test_one_peer_without_the_comb(trio, world, oracle):
    """BLS_DEBUG_NO_PK_COMB on the peer only: it does not pass the row pointers; verdicts
    equal the owner's and the partial records are equal byte for byte"""
    keys = list(range(5, 70))
    sets, outcomes, good = world.call65(keys, b"nocomb-")
    trio.peer.base_debug_flags = FLAGS | DEBUG_NO_PK_COMB
    trio.peer.set_debug_flags(0)
    try:
        _check(oracle, trio.all()[:2], sets, outcomes)
        assert _partial(trio.owner, good) == _partial(trio.peer, good)
    finally:
        trio.peer.base_debug_flags = FLAGS
        trio.peer.set_debug_flags(0)


def test_refusals(trio):
    """sharing into a context that holds keys and sharing with itself return -2 with a
    message; a repeated share returns 0.  (The different-device refusal needs two GPUs.)"""
    lib = trio.owner.lib
    before = trio.private.pubkeys_info()
    assert lib.bls_gpu_share_pubkeys(trio.private._h, trio.owner._h) == -2
    assert b"holds" in lib.bls_gpu_last_error(trio.private._h)
    assert trio.private.pubkeys_info() == before
    assert lib.bls_gpu_share_pubkeys(trio.owner._h, trio.owner._h) == -2
    assert b"itself" in lib.bls_gpu_last_error(trio.owner._h)
    assert lib.bls_gpu_share_pubkeys(trio.owner._h, None) == -2
    with pytest.raises(NativeError):
        trio.private.share_pubkeys(trio.peer)
    assert lib.bls_gpu_share_pubkeys(trio.peer._h, trio.owner._h) == 0
    assert lib.bls_gpu_share_pubkeys(trio.owner._h, trio.peer._h) == 0
    assert trio.owner.pubkeys_info()["n_contexts"] == 2


def test_the_cache_line_shared_by_the_last_key_and_the_next(world):
    """with 100-B entries key 73 begins 4 bytes into the line that ends key 72.  With the
    table at 73 keys the owner verifies a set on key 72, the peer appends one key, and the
    owner then verifies a valid set on key 73 -- as does a fourth context that shares only
    then.  The same pair then takes a batch holding an undecodable key through the peer:
    n_keys stays on both, and the next good batch lands at the old index."""
    assert (73 * ENTRY - 1) // 128 == (73 * ENTRY) // 128 and (73 * ENTRY) % 128 == 4
    owner, peer = _pair(world)
    late = None
    try:
        s72, s73, s74, s75 = world.sets([72, 73, 74, 75], b"line-")
        assert _verify(owner, [s72])[0] == [1]
        assert _verify(owner, [s73])[0] != [1]  # (not there yet)
        _load(peer, world.blob(73, 1))
        assert _verify(owner, [s73])[0] == [1]
        assert _verify(owner, [s72, s73])[0] == [1, 1]
        late = _ctx()
        late.share_pubkeys(peer)
        assert _verify(late, [s73])[0] == [1]
        assert late.pubkeys_info()["n_contexts"] == 3
        # all or nothing, for all sharers
        codes = peer.load_pubkeys(world.blob(74, 1) + b"\xff" * 48 + world.blob(75, 1), 48)
        assert list(codes != 0) == [False, True, False]
        assert [c.pubkeys_info()["n_keys"] for c in (owner, peer, late)] == [74] * 3
        assert _verify(owner, [s74])[0] != [1]
        _load(peer, world.blob(74, 2))
        assert [c.pubkeys_info()["n_keys"] for c in (owner, peer, late)] == [76] * 3
        for c in (owner, late):
            assert _verify(c, [s74, s75, s72])[0] == [1, 1, 1]
    finally:
        for c in (owner, peer, late):
            if c is not None:
                c.close()


def test_appends_during_calls(world, oracle):
    """one thread runs eight 65-set calls on the owner over keys loaded before the threads
    start (one set invalid); another appends batches through the peer that grow the table
    at least twice.  Every verdict array is the expected one whatever the interleaving;
    afterwards a call over the newest keys passes on both contexts."""
    owner, peer = _pair(world)
    try:
        sets, outcomes, _ = world.call65(list(range(0, 65)), b"during-")
        want, retries, ok = _expected(oracle, outcomes)
        # the appended indices 73 + j hold key 73 + j % 1000 (the third load's first 1,000 keys, repeated)
        batches = [world.blob(N1 + N2, 1000), world.blob(N1 + N2, 1000), world.blob(N1 + N2, 600)]
        total = N1 + N2 + 2600
        newest = world.call65(list(range(total - 65, total)), b"newest-", lambda k: 73 + (k - 73) % 1000)[0]
        newest[40] = world.sets([total - 25], b"n40-", lambda k: 73 + (k - 73) % 1000)[0]  # all 65 valid
        got, caps, errors = [], [owner.pubkeys_info()["capacity"]], []

        def calls():
            try:
                for _ in range(8):
                    got.append(_verify(owner, sets))
            except Exception as e:  # noqa: BLE001 - reported by the test's thread
                errors.append(e)

        def appends():
            try:
                for blob in batches:
                    _load(peer, blob)
                    caps.append(peer.pubkeys_info()["capacity"])
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=calls), threading.Thread(target=appends)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert len(got) == 8
        for v, st in got:
            assert v == want
            assert (st.batch_retries, st.batch_sigs_success) == (retries, ok)
        assert len(set(caps)) >= 3, caps  # two growths
        assert owner.pubkeys_info() == peer.pubkeys_info() and owner.pubkeys_info()["n_keys"] == total
        for c in (owner, peer):
            assert _verify(c, newest)[0] == [1] * 65
    finally:
        owner.close()
        peer.close()


def test_the_owner_closes_first(world, oracle):
    """the table lives until its last context closes: the peer keeps verifying and appending"""
    owner, peer = _pair(world)
    try:
        assert peer.pubkeys_info()["n_contexts"] == 2
        owner.close()
        info = peer.pubkeys_info()
        assert (info["n_contexts"], info["n_keys"]) == (1, N1 + N2)
        sets, outcomes, _ = world.call65(list(range(8, 73)), b"orphan-")
        _check(oracle, [("peer", peer)], sets, outcomes)
        _load(peer, world.blob(N1 + N2, 10))
        assert peer.pubkeys_info()["n_keys"] == N1 + N2 + 10
        assert _verify(peer, world.sets([80, 82, 0], b"orphan2-"))[0] == [1, 1, 1]
    finally:
        peer.close()


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
from lodestar_amd._abi import DEBUG_MERGED_EVERY_PASS, DEBUG_SIGAGG_ON
from lodestar_amd.native import GpuContext, pack_requests
from oracle import bls_oracle as O
n = int(sys.argv[2])
sks = [O.interop_secret_key(i).to_bytes(32, "big") for i in range(n)]
with GpuContext(0) as owner, GpuContext(0) as peer:
    for c in (owner, peer):
        c.base_debug_flags = DEBUG_SIGAGG_ON | DEBUG_MERGED_EVERY_PASS
        c.set_debug_flags(0)
    peer.share_pubkeys(owner)
    assert (owner.load_pubkeys(owner.sk_to_pk(b"".join(sks)).tobytes(), 48) == 0).all()
    keys = list(range(n - 65, n))
    msgs = [hashlib.sha256(b"cap-%d" % i).digest() for i in range(65)]
    sigs = owner.sign(b"".join(sks[k] for k in keys), b"".join(msgs))
    sets = [([k], m, s.tobytes()) for k, m, s in zip(keys, msgs, sigs)]
    sets[64] = (sets[64][0], msgs[0], sets[64][2])
    v, st = peer.verify_packed(pack_requests([(True, [s]) for s in sets], seed=bytes(32)))
    print(json.dumps({"v": [int(x) for x in v], "retries": st.batch_retries, "ok": st.batch_sigs_success,
                      "owner": owner.pubkeys_info(), "peer": peer.pubkeys_info()}))
"""


def test_the_rows_cap_is_per_table_in_a_child_process(oracle):
    """BLS_PK_COMB_MAX_MB=1 on a shared pair: 728 keys get rows (1 MiB / 1,440 B), once; a
    65-set call over keys 695..759 through the peer straddles the cap (33 sets on rows, 32 on
    the GLV chain), one set signed for another message"""
    n = 760
    assert (1 << 20) // ROWS == 728 and n - 65 < 728 < n
    env = dict(os.environ, BLS_PK_COMB_MAX_MB="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), str(n)], capture_output=True, text=True,
                         timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    want, retries, ok = _expected(oracle, [0 if i == 64 else 1 for i in range(65)])
    assert got["v"] == want
    assert (got["retries"], got["ok"]) == (retries, ok)
    assert got["owner"] == got["peer"]
    info = got["peer"]
    cap = n + n // 2 + 1024
    assert (info["n_keys"], info["comb_keys"], info["capacity"], info["n_contexts"]) == (n, 728, cap, 2)
    assert info["device_bytes"] == cap * ENTRY + 728 * (ROWS + 1)


def test_the_python_verifier_shares_by_default(world):
    """GpuBlsVerifier(n_contexts=3): one table_id over its four contexts; a batchable job and
    a same-message job verify; load_pubkeys after the start appends once and the new keys
    verify on the pool and on the main-thread lane; with share_pubkeys=False there are four
    ids"""
    from lodestar_amd.verifier import GpuBlsVerifier, SignatureSet

    def sig_sets(sets):
        return [SignatureSet(k[0], m, s) for k, m, s in sets]

    first = world.sets(list(range(0, 40)), b"verifier-")
    later = world.sets(list(range(73, 83)), b"verifier-later-")
    msg = _h(b"verifier same message")
    sm_keys = list(range(40, 60))
    sm_sigs = world.gpu.sign(b"".join(world.sks[k] for k in sm_keys), msg * len(sm_keys))
    v = GpuBlsVerifier(n_contexts=3, pubkeys48=world.blob(0, N1 + N2))
    try:
        ctxs = [v._main] + v._ctxs
        assert len(ctxs) == 4
        infos = [c.pubkeys_info() for c in ctxs]
        assert len({i["table_id"] for i in infos}) == 1
        assert infos[0]["n_contexts"] == 4 and infos[0]["n_keys"] == N1 + N2
        assert v.verify_signature_sets(sig_sets(first), batchable=True) is True
        bad = sig_sets(first[:4])
        bad[2] = SignatureSet(bad[2].pubkey, _h(b"not signed"), bad[2].signature)
        assert v.verify_signature_sets(bad, batchable=True) is False
        assert v.verify_signature_sets(sig_sets(first[:3]), verify_on_main_thread=True) is True
        assert v.verify_signature_sets_same_message([(k, s.tobytes()) for k, s in zip(sm_keys, sm_sigs)], msg) \
            == [True] * len(sm_keys)
        v.load_pubkeys(world.blob(N1 + N2, 10))
        assert [c.pubkeys_info()["n_keys"] for c in ctxs] == [N1 + N2 + 10] * 4  # one append, seen by all
        assert v.verify_signature_sets(sig_sets(later), batchable=True) is True
        assert v.verify_signature_sets(sig_sets(later[:2]), verify_on_main_thread=True) is True
        with pytest.raises(Exception, match="no key appended"):
            v.load_pubkeys(world.blob(0, 1) + b"\xff" * 48)
        assert [c.pubkeys_info()["n_keys"] for c in ctxs] == [N1 + N2 + 10] * 4
    finally:
        v.close()
    own = GpuBlsVerifier(n_contexts=3, pubkeys48=world.blob(0, N1 + N2), share_pubkeys=False)
    try:
        infos = [c.pubkeys_info() for c in [own._main] + own._ctxs]
        assert len({i["table_id"] for i in infos}) == 4
        assert all(i["n_contexts"] == 1 and i["n_keys"] == N1 + N2 for i in infos)
        assert own.verify_signature_sets(sig_sets(first[:5]), batchable=True) is True
    finally:
        own.close()
