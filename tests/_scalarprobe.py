"""CPU-only construction of the cancelling-forgery probes of tests/test_gpu_scalar_probe.py
(proved by tests/test_scalarprobe_cpu.py against the oracle): batches that are invalid set
by set, but whose random-scalar batch equation holds exactly when the library multiplies
the sets at two chosen positions by the group scalars rho_a : rho_b it documents.

The derivation, written down here independently of the code under test (hashlib and
integers only; bls/pipeline.hpp set_scalar, bls/curve.hpp glv_split):

  block(seed) = the seed's eight 4-byte words in reverse order (bytes 28..31 first)
  r64(seed, i) = BE64(SHA-256(block(seed) || LE32(i))[0:8]), 0 -> 1
  a, b         = the low and the high 32 bits of r64
  rho(seed, i) = (a + b mu) mod r,   mu = -x^2 mod r

Nothing here touches the GPU library or the CPU build of its stage bodies."""
from __future__ import annotations

import functools
import hashlib

from oracle import bls_oracle as O

R = O.R
MU = (-(O.X_ABS * O.X_ABS)) % R
CHUNK_MIN = 16  # worker.ts:17 MAX_SIGNATURE_SETS_PER_JOB's chunkify floor


def seed_block(seed: bytes) -> bytes:
    """what set_scalar hashes in front of the index: the 32-byte seed word-reversed"""
    assert len(seed) == 32
    return b"".join(seed[28 - 4 * k: 32 - 4 * k] for k in range(8))


def r64(seed: bytes, i: int) -> int:
    d = hashlib.sha256(seed_block(seed) + (i & 0xFFFFFFFF).to_bytes(4, "little")).digest()
    return int.from_bytes(d[:8], "big") or 1


def halves(v: int) -> tuple[int, int]:
    return v & 0xFFFFFFFF, v >> 32


def rho_of(v: int) -> int:
    a, b = halves(v)
    return (a + b * MU) % R


def rho(seed: bytes, i: int, flip_bit: int | None = None) -> int:
    """the group scalar of set index i; flip_bit: the control's, one bit of r64 flipped
    before the scalar is formed"""
    v = r64(seed, i)
    if flip_bit is not None:
        v ^= 1 << flip_bit
        assert v != 0
    return rho_of(v)


def find_seed(index: int, predicate, cap: int = 1 << 22) -> bytes:
    """the first seed sha256(b"scalarprobe" || LE32(c)), c = 0, 1, ..., whose scalar halves
    (a, b) at `index` satisfy predicate(a, b); raises at the cap (a condition on the inputs:
    every predicate in use has probability >= 2^-16)"""
    for c in range(cap):
        seed = hashlib.sha256(b"scalarprobe" + c.to_bytes(4, "little")).digest()
        if predicate(*halves(r64(seed, index))):
            return seed
    raise AssertionError("find_seed: no seed below the cap %d" % cap)


# scalar shapes of section 6: the skipped-addition / accumulator-still-infinity branches of
# curve.hpp jac_mul_glv (joint 2-bit windows from the top) and g1_comb_mul (digit j of a
# half is bits j, 8 + j, 16 + j, 24 + j; j = 7 is the leading one)
SHAPES = {
    "top_window_zero": lambda a, b: a >> 30 == 0 and b >> 30 == 0,
    "leading_comb_digit_zero": lambda a, b: (a | b) & 0x80808080 == 0,
    "a_below_65536": lambda a, b: a < 1 << 16,
    "b_below_65536": lambda a, b: b < 1 << 16,
}


@functools.lru_cache(maxsize=None)
def shape_seed(shape: str, index: int) -> bytes:
    return find_seed(index, SHAPES[shape])


# ---------------------------------------------------------------------------
# the cancelling pairs
# ---------------------------------------------------------------------------
def cancelling_sks(sk_a: int, sk_b: int, rho_a: int, rho_b: int, d: int) -> tuple[int, int]:
    """(sk_a + rho_b d, sk_b - rho_a d) mod r: rho_a sk_a' + rho_b sk_b' = rho_a sk_a + rho_b
    sk_b.  Signing one shared root with them is the signature-side pair (sig' = sig +- [rho]
    [d]H(m)); their public keys are the key-side pair."""
    assert d % R != 0
    return (sk_a + rho_b * d) % R, (sk_b - rho_a * d) % R


@functools.lru_cache(maxsize=None)
def _d_powers(d_tag: bytes):
    """[2^i]D, i < 255, for D = hash_to_g2(d_tag) (in G2, of unknown discrete log to every
    H(m)): made once, so that a multiple of D costs additions only"""
    out = [O.hash_to_g2(hashlib.sha256(d_tag).digest())]
    for _ in range(254):
        out.append(O.E2.add(out[-1], out[-1]))
    return out


@functools.lru_cache(maxsize=None)
def _mul_d(d_tag: bytes, k: int):
    """[k]D with the oracle's additions"""
    acc, k = None, k % R
    for i, p in enumerate(_d_powers(d_tag)):
        if (k >> i) & 1:
            acc = O.E2.add(acc, p)
    return acc


def cancelling_sigs(sig_a: bytes, sig_b: bytes, rho_a: int, rho_b: int, d_tag: bytes = b"scalarprobe D"):
    """(sig_a + [rho_b]D, sig_b - [rho_a]D) compressed: the general signature-side pair,
    for sets on different roots"""
    pa, pb = O.signature_from_bytes(sig_a, validate=False), O.signature_from_bytes(sig_b, validate=False)
    return (O.g2_compress(O.E2.add(pa, _mul_d(d_tag, rho_b))),
            O.g2_compress(O.E2.add(pb, O.E2.neg(_mul_d(d_tag, rho_a)))))


@functools.lru_cache(maxsize=None)
def pk48(sk: int) -> bytes:
    return O.g1_compress(O.sk_to_pk(sk))


@functools.lru_cache(maxsize=None)
def pk96(sk: int) -> bytes:
    return O.g1_serialize(O.sk_to_pk(sk))


# ---------------------------------------------------------------------------
# the expected outcome of a call
# ---------------------------------------------------------------------------
class Pair:
    """sets a and b (set indices of the call) form a cancelling pair: each invalid alone,
    valid together where one check covers both -- unless it is the control"""

    def __init__(self, a: int, b: int, cancels: bool = True):
        self.a, self.b, self.cancels = a, b, cancels


def _scope_ok(scope, pairs, invalid) -> bool:
    s = set(scope)
    if s & set(invalid):
        return False
    for p in pairs:
        ina, inb = p.a in s, p.b in s
        if (ina or inb) and not (ina and inb and p.cancels):
            return False
    return True


def expected_call(req_sets, batchable, pairs=(), invalid=(), merged: bool = True, bounds=None):
    """(verdicts, batch_retries, batch_sigs_success, merged_check) of one verify call from
    its check scopes: a pair cancels exactly when both members are inside one scope.

      req_sets   per request its set indices; batchable: per request
      merged     the merged check runs where the pass is eligible (only batchable requests
                 and at least two chunks): its scope is the whole pass; merged_check is 1 /
                 2 (passed / failed) or 0 (not run)
      bounds     bls_gpu_verify_many: the first request of each message (chunks never span
                 two messages); None: one message
    The chunks are oracle.chunkify_maximize_chunk_size's (a scope each); a request of a
    failed chunk and a non-batchable request are a scope each.  A cancelling pair split over
    two requests of one chunk that fails for another reason is outside the model (the
    reference retries the requests alone, the group tests may check them together) and
    raises."""
    n_req = len(req_sets)
    bounds = list(bounds or [0]) + [n_req]
    chunks = []
    for m in range(len(bounds) - 1):
        msg_b = [r for r in range(bounds[m], bounds[m + 1]) if batchable[r]]
        if msg_b:
            chunks += O.chunkify_maximize_chunk_size(msg_b, CHUNK_MIN)
    nonbatch = [r for r in range(n_req) if not batchable[r]]
    verdicts = [None] * n_req
    retries = ok_sets = 0
    sets_of = lambda reqs: [i for r in reqs for i in req_sets[r]]
    merged_check = 0
    chunk_ok = None
    if merged and not nonbatch and len(chunks) >= 2:
        if _scope_ok(sets_of(range(n_req)), pairs, invalid):
            merged_check, chunk_ok = 1, [True] * len(chunks)
        else:
            merged_check = 2
    if chunk_ok is None:
        chunk_ok = [_scope_ok(sets_of(c), pairs, invalid) for c in chunks]
    alone = list(nonbatch)
    for c, ok in zip(chunks, chunk_ok):
        if ok:
            for r in c:
                verdicts[r] = 1
                ok_sets += len(req_sets[r])
        else:
            retries += 1
            for p in pairs:
                ra = [r for r in c if p.a in req_sets[r]]
                rb = [r for r in c if p.b in req_sets[r]]
                if p.cancels and ra and rb and ra != rb:
                    raise AssertionError("a cancelling pair split over requests of a failed chunk is not modelled")
            alone += c
    for r in alone:
        verdicts[r] = 1 if _scope_ok(req_sets[r], pairs, invalid) else 0
    return verdicts, retries, ok_sets, merged_check
