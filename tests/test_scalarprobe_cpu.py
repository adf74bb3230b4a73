"""The batch scalars in writing, and the cancelling-forgery probes of tests/_scalarprobe.py
proved on the CPU before tests/test_gpu_scalar_probe.py feeds them to the device:

  * bls/pipeline.hpp set_scalar (through tests/native/hostsim.cpp hs_set_scalar) equals
    the hashlib formula r64 at indices that exercise every byte of the hashed index;
  * a probe is invalid set by set, passes the oracle's verify_multiple under the group
    scalars rho = a + b mu and fails it under the raw 64-bit values; its control (one bit
    of r_b flipped before rho_b is formed) fails;
  * the same pairs through hs_verify_batch, the CPU build of the stage bodies
    (stage_scale / stage_chunk / stage_indiv)."""
from __future__ import annotations

import ctypes
import functools
import hashlib

import pytest

from oracle import bls_oracle as O
from tests import _scalarprobe as sp
from tests.test_hostsim import _hs_verify

SEED = bytes(range(32))
SEEDS = (SEED, bytes(32), hashlib.sha256(b"scalarprobe seed").digest())
INDICES = (0, 1, 255, 256, 65535, 65536, 0x01020304, 0xFFFFFFFF)
A, B = 0, 2  # the probed positions of the 3-set batches


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def test_issue_known_values():
    """the values recorded when the derivation was read off the code: seed 00 01 .. 1f,
    index 0; the documented-but-wrong formula (the seed as it stands) gives another"""
    assert "%016x" % sp.r64(SEED, 0) == "b351dd56cfc98dc5"
    assert hashlib.sha256(SEED + bytes(4)).digest()[:8].hex() == "70f4003d52b6eb03"
    assert sp.MU == (-(0xD201000000010000 ** 2)) % sp.R
    assert (sp.MU * sp.MU + sp.MU + 1) % sp.R == 0  # a primitive cube root of unity mod r


@pytest.mark.parametrize("k", range(len(SEEDS)))
def test_set_scalar_matches_hashlib(hostsim, k):
    hostsim.hs_set_scalar.restype = ctypes.c_uint64
    hostsim.hs_set_scalar.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    for i in INDICES:
        got = hostsim.hs_set_scalar(SEEDS[k], i)
        assert got == sp.r64(SEEDS[k], i), "seed %d, index %#x: %016x" % (k, i, got)
    vals = {sp.r64(SEEDS[k], i) for i in INDICES}
    assert len(vals) == len(INDICES)  # every byte of the index reaches the hash


def test_find_seed_shapes():
    for name, pred in sp.SHAPES.items():
        a, b = sp.halves(sp.r64(sp.shape_seed(name, 1), 1))
        assert pred(a, b), name
    with pytest.raises(AssertionError):
        sp.find_seed(0, lambda a, b: False, cap=8)


@pytest.fixture(scope="module")
def base(oracle):
    """three valid sets: 0 and 2 sign one shared root, 1 its own; and three on distinct roots"""
    sks = [oracle.interop_secret_key(i) for i in range(3)]
    shared = [_h(b"sp shared"), _h(b"sp own 1"), _h(b"sp shared")]
    distinct = [_h(b"sp distinct %d" % i) for i in range(3)]
    return sks, shared, distinct


@functools.lru_cache(maxsize=None)
def _sign(sk: int, msg: bytes) -> bytes:
    return O.g2_compress(O.sign(sk, msg))


@functools.lru_cache(maxsize=None)
def _pk(sk: int):
    return O.sk_to_pk(sk)


def _sets(oracle, sks, msgs, key_sks=None):
    return [(_pk(k), m, _sign(s, m)) for s, m, k in zip(sks, msgs, key_sks or sks)]


def _rhos(bit=None):
    return [sp.rho(SEED, 0), sp.rho(SEED, 1), sp.rho(SEED, 2, bit)]


def _sig_side_shared(oracle, base, bit=None):
    """signature-side pair on the shared root, by secret keys alone"""
    sks, shared, _ = base
    ra, _, rb = _rhos(bit)
    sa, sb = sp.cancelling_sks(sks[A], sks[B], ra, rb, 0x1234567)
    return _sets(oracle, [sa, sks[1], sb], shared, key_sks=sks)


def _sig_side_general(oracle, base, bit=None):
    """signature-side pair on different roots, by D"""
    sks, _, distinct = base
    sets = _sets(oracle, sks, distinct)
    ra, _, rb = _rhos(bit)
    sig_a, sig_b = sp.cancelling_sigs(sets[A][2], sets[B][2], ra, rb)
    return [(sets[0][0], distinct[0], sig_a), sets[1], (sets[2][0], distinct[2], sig_b)]


def _key_side(oracle, base, bit=None):
    """key-side pair: the original valid signatures, edited keys"""
    sks, shared, _ = base
    ra, _, rb = _rhos(bit)
    ka, kb = sp.cancelling_sks(sks[A], sks[B], ra, rb, 0x7654321)
    return _sets(oracle, sks, shared, key_sks=[ka, sks[1], kb])


_BUILDERS = {"sig_shared_root": _sig_side_shared, "sig_general_D": _sig_side_general, "key_side": _key_side}


@pytest.mark.parametrize("kind", list(_BUILDERS))
def test_construction_against_oracle(oracle, base, kind):
    """probe: True under rho, False under the raw 64-bit values, the edited sets False
    alone; control (bit 32 of r_b flipped): False under rho"""
    probe = _BUILDERS[kind](oracle, base)
    true_rho = _rhos()
    assert oracle.verify_multiple(probe, scalars=true_rho) is True
    assert oracle.verify_multiple(probe, scalars=[sp.r64(SEED, i) for i in range(3)]) is False
    assert oracle.core_verify(*probe[A]) is False
    assert oracle.core_verify(*probe[B]) is False
    assert oracle.core_verify(*probe[1]) is True
    control = _BUILDERS[kind](oracle, base, bit=32)
    assert oracle.verify_multiple(control, scalars=true_rho) is False
    assert oracle.core_verify(*control[A]) is False


@pytest.fixture(scope="module")
def hs_table(hostsim, oracle, base):
    """the harness's table: interop keys 0..2, then the key-side probe's and its controls'
    edited keys (index by secret key)"""
    sks = base[0]
    ra, _, rb = _rhos()
    keys = list(sks)
    for bit in (None, 0, 31, 32, 63):
        keys += sp.cancelling_sks(sks[A], sks[B], ra, sp.rho(SEED, B, bit), 0x7654321)
    keys = list(dict.fromkeys(keys))
    hostsim.hs_clear_pubkeys()
    assert hostsim.hs_load_pubkeys(b"".join(sp.pk48(k) for k in keys), len(keys), 48, None) == len(keys)
    yield {k: i for i, k in enumerate(keys)}
    hostsim.hs_clear_pubkeys()


def _table_sets(oracle, base, hs_table, kind, bit=None):
    """the builders' sets with table indices for keys"""
    sets = _BUILDERS[kind](oracle, base, bit)
    sks = base[0]
    key_sks = list(sks)
    if kind == "key_side":
        ra, _, rb = _rhos(bit)
        key_sks[A], key_sks[B] = sp.cancelling_sks(sks[A], sks[B], ra, rb, 0x7654321)
    return [([hs_table[k]], m, sig) for k, (_, m, sig) in zip(key_sks, sets)]


@pytest.mark.parametrize("kind", list(_BUILDERS))
def test_probe_through_stage_bodies(hostsim, oracle, base, hs_table, kind):
    """hs_verify_batch: probe and controls as one-set batchable requests in one chunk (sets
    a and b get 0 after the fallback for a control, everything 1 for the probe), and the
    probe inside one non-batchable 3-set request"""
    probe = _table_sets(oracle, base, hs_table, kind)
    v, st = _hs_verify(hostsim, [(True, [s]) for s in probe], seed=SEED)
    assert (v, st.batch_retries, st.batch_sigs_success) == ([1, 1, 1], 0, 3), kind
    v, _ = _hs_verify(hostsim, [(False, probe)], seed=SEED)
    assert v == [1], kind
    v, _ = _hs_verify(hostsim, [(False, [s]) for s in probe], seed=SEED)
    assert v == [0, 1, 0], kind
    for bit in (0, 31, 32, 63):
        control = _table_sets(oracle, base, hs_table, kind, bit)
        v, st = _hs_verify(hostsim, [(True, [s]) for s in control], seed=SEED)
        assert (v, st.batch_retries, st.batch_sigs_success) == ([0, 1, 0], 1, 0), (kind, bit)
    v, _ = _hs_verify(hostsim, [(False, _table_sets(oracle, base, hs_table, kind, 63))], seed=SEED)
    assert v == [0], kind


def test_expected_call_model():
    """the outcome model on the layouts the GPU tests use"""
    one = lambda n: [[i] for i in range(n)]
    # one chunk of 20: the pair cancels in it; the control fails it
    assert sp.expected_call(one(20), [True] * 20, [sp.Pair(3, 17)]) == ([1] * 20, 0, 20, 0)
    want = [0 if i in (3, 17) else 1 for i in range(20)]
    assert sp.expected_call(one(20), [True] * 20, [sp.Pair(3, 17, False)]) == (want, 1, 0, 0)
    # two chunks of 16, the pair across them: the merged pass covers both
    assert sp.expected_call(one(32), [True] * 32, [sp.Pair(3, 20)]) == ([1] * 32, 0, 32, 1)
    want = [0 if i in (3, 20) else 1 for i in range(32)]
    assert sp.expected_call(one(32), [True] * 32, [sp.Pair(3, 20)], merged=False) == (want, 2, 0, 0)
    # the pair in chunk 0, an invalid set in chunk 1
    want = [0 if i == 25 else 1 for i in range(32)]
    assert sp.expected_call(one(32), [True] * 32, [sp.Pair(3, 9)], invalid=[25]) == (want, 1, 16, 2)
    # verify_many 17 + 5 + 19: one chunk per message
    want = [1] * 41
    assert sp.expected_call(one(41), [True] * 41, [sp.Pair(3, 30)], bounds=[0, 17, 22]) == (want, 0, 41, 1)
    want = [0 if i in (3, 30) else 1 for i in range(41)]
    assert sp.expected_call(one(41), [True] * 41, [sp.Pair(3, 30, False)], bounds=[0, 17, 22]) == (want, 2, 5, 2)
    # a non-batchable request holding the pair, alone and among one-set requests
    assert sp.expected_call([[0, 1, 2]], [False], [sp.Pair(0, 2)]) == ([1], 0, 0, 0)
    assert sp.expected_call([[0, 1, 2]], [False], [sp.Pair(0, 2, False)]) == ([0], 0, 0, 0)
