"""Point encodings at the field and flag-byte edges through every GPU entry point that
takes bytes from outside (the decoders g2_decompress96, g1_decompress48, g1_deserialize96
of csrc/bls/curve.hpp, compiled for the device with the inline-asm carry chains).

The vectors are tests/_wirevec.py's: non-canonical aliases x + p of valid signatures and
keys (the one input a decoder that reduces mod p answers with 1), p +- 2^(32k) in every
limb, the flag bits, stray bytes on infinity, and E2 points with y.c1 == 0 / y.c0 == 0.
Every expected code, point and verdict is the oracle's (oracle/bls_oracle.py); every
comparison is exact and a failure names its vector.  tests/test_wirevec_cpu.py runs the
same vectors through the CPU build of the same headers."""
from __future__ import annotations

import contextlib
import functools
import hashlib

import pytest

from lodestar_amd._abi import DEBUG_MERGED_EVERY_PASS, DEBUG_SIGAGG_OFF, DEBUG_SIGAGG_ON
from lodestar_amd.deposits import deposit_domain
from lodestar_amd.native import GpuContext, pack_deposits, pack_requests
from oracle import ssz_oracle
from tests import _wirevec as W
from tests._codec import g1b, g2b

pytestmark = pytest.mark.gpu

E_OK, E_BAD = 0, 1
INF_G2_192 = bytes([0x40]) + bytes(191)  # k_g2_decompress's output for every code != 0
INF_SIG96 = bytes([0xC0]) + bytes(95)
N_TABLE = 16
SEED = bytes(range(64, 96))
DOMAIN = deposit_domain(bytes.fromhex("00000001"))
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def _sk(oracle, i: int) -> bytes:
    return oracle.interop_secret_key(i).to_bytes(32, "big")


@pytest.fixture(scope="module")
def ctx(golden):
    """a context of this module's own; its table holds the first 16 interop keys"""
    c = GpuContext(0)
    pks = b"".join(bytes.fromhex(h) for h in golden["kat2_interop_pubkeys"][:N_TABLE])
    assert (c.load_pubkeys(pks, 48) == 0).all()
    yield c
    c.close()


PATHS = {"pset": DEBUG_SIGAGG_OFF, "sigagg": DEBUG_SIGAGG_ON}


@contextlib.contextmanager
def _forced(c, flags: int):
    """the context with a per-set verify path forced (tests/test_gpu_parity.py verify_path),
    for one call"""
    c.set_debug_flags(flags | DEBUG_MERGED_EVERY_PASS)
    try:
        yield
    finally:
        c.set_debug_flags(0)


# ---- bls_gpu_g2_decompress ---------------------------------------------------------------------
@pytest.mark.parametrize("validate", [False, True])
def test_g2_decompress(gpu, validate):
    vecs = W.g2_vectors()
    out, codes = gpu.g2_decompress(b"".join(v.data for v in vecs), validate=validate)
    assert len(codes) == len(vecs)
    for v, row, code in zip(vecs, out, codes):
        want = v.vcode if validate else v.code
        assert int(code) == want, "%s: code %d, oracle %d" % (v.name, code, want)
        want_bytes = g2b(v.point) if want == E_OK else INF_G2_192
        assert row.tobytes() == want_bytes, "%s: point %s, want %s" % (v.name, row.tobytes().hex(), want_bytes.hex())


# ---- bls_gpu_aggregate_signatures --------------------------------------------------------------
def test_aggregate_signatures_single_element_lists(gpu):
    vecs = W.g2_vectors()
    out, codes = gpu.aggregate_signatures([[v.data] for v in vecs])
    for v, o, code in zip(vecs, out, codes):
        assert int(code) == v.vcode, "%s: code %d, oracle %d" % (v.name, code, v.vcode)
        if v.vcode == E_OK:  # the sum of one point is the point: the bytes that went in
            assert o == v.data, "%s: sum %s" % (v.name, o.hex())


def test_aggregate_signatures_alias_inside_a_list(gpu):
    g2 = W.by_name(W.g2_vectors())
    members = [g2["canon"], g2["alias_c0"], g2["sort_flip"]]
    assert [m.vcode for m in members] == [E_OK, E_BAD, E_OK]
    out, codes = gpu.aggregate_signatures([[m.data for m in members]])
    assert int(codes[0]) == E_BAD and out[0] == INF_SIG96


# ---- the per-set verify paths --------------------------------------------------------------------
VERIFY_VECTORS = ("alias_c0", None, "alias_c1", None, "sort_flip", "c0_high_bits/bit7", "c0=p", "precedence",
                  "flags_e0/s0_body", "flags_00/s0_body")


@functools.lru_cache(maxsize=None)
def _sort_flip_is_no_signature() -> bool:
    """oracle.core_verify on sort_flip = -S0 under key 0 and S0's message (one pairing check
    in pure Python, done once)"""
    from oracle import bls_oracle as O

    pk0 = O.sk_to_pk(O.interop_secret_key(0))
    return O.core_verify(pk0, W.msg_of(W.S0_INDEX), W.by_name(W.g2_vectors())["sort_flip"].data) is False


def _valid_sets(ctx, oracle, keys, tag: bytes):
    msgs = [_h(tag + b"%d" % k) for k in keys]
    sigs = ctx.sign(b"".join(_sk(oracle, k) for k in keys), b"".join(msgs))
    return [([k], m, s.tobytes()) for k, m, s in zip(keys, msgs, sigs)]


@pytest.mark.parametrize("batchable", [False, True])
@pytest.mark.parametrize("verify_path", list(PATHS))
def test_verify_one_set_requests(ctx, oracle, verify_path, batchable):
    """one call of one-set requests: every edge signature between valid neighbours.  The
    edge signatures are key 0's over the message they were made for (alias_c1 over S1's)."""
    g2 = W.by_name(W.g2_vectors())
    valid = iter(_valid_sets(ctx, oracle, range(1, 8), b"wire-edge-"))
    names, sets, want = ["valid"], [next(valid)], [1]
    for nm in VERIFY_VECTORS:
        if nm is None:
            names.append("valid")
            sets.append(next(valid))
            want.append(1)
            continue
        v = g2[nm]
        msg = W.msg_of(W.S1_INDEX if nm == "alias_c1" else W.S0_INDEX)
        names.append(nm)
        sets.append(([0], msg, v.data))
        want.append(-v.vcode)  # a decode or group error: -code; else a point that is no signature here
    assert [w for w in want if w == 0] == [0] and want[names.index("sort_flip")] == 0
    assert _sort_flip_is_no_signature()
    assert all(want[names.index(nm)] == -E_BAD for nm in VERIFY_VECTORS if nm not in (None, "sort_flip"))
    with _forced(ctx, PATHS[verify_path]):
        got, _ = ctx.verify_packed(pack_requests([(batchable, [s]) for s in sets], seed=SEED))
    for nm, g, w in zip(names, got, want):
        assert int(g) == w, "%s (%s, batchable=%s): verdict %d, want %d" % (nm, verify_path, batchable, g, w)


@pytest.mark.parametrize("verify_path", list(PATHS))
def test_verify_two_set_request_with_alias(ctx, oracle, verify_path):
    g2 = W.by_name(W.g2_vectors())
    first = _valid_sets(ctx, oracle, [1], b"wire-two-")[0]
    second = ([0], W.msg_of(W.S0_INDEX), g2["alias_c0"].data)
    pk = [oracle.sk_to_pk(oracle.interop_secret_key(k)) for k in (1, 0)]
    res, _, _ = oracle.verify_many_signature_sets([(False, [(pk[0], first[1], first[2]), (pk[1], second[1], second[2])])])
    assert res[0][0] == "error" and res[0][1].code == E_BAD
    with _forced(ctx, PATHS[verify_path]):
        got, _ = ctx.verify_packed(pack_requests([(False, [first, second]), (False, [first])], seed=SEED))
    assert [int(x) for x in got] == [-res[0][1].code, 1], "alias_c0 as the second set (%s)" % verify_path


# ---- bls_gpu_verify_same_message ---------------------------------------------------------------
def test_verify_same_message(ctx, oracle):
    """six sets over S0's message: key 0's alias_c0 at position 2, key 0's sort_flip at 4"""
    g2 = W.by_name(W.g2_vectors())
    msg = W.msg_of(W.S0_INDEX)
    keys = [1, 2, 0, 3, 0, 4]
    sigs = [s.tobytes() for s in ctx.sign(b"".join(_sk(oracle, k) for k in keys), msg * 6)]
    assert sigs[2] == g2["canon"].data  # the device signs what the oracle signs
    sigs[2], sigs[4] = g2["alias_c0"].data, g2["sort_flip"].data
    assert g2["alias_c0"].vcode == E_BAD and g2["sort_flip"].vcode == E_OK and _sort_flip_is_no_signature()
    got, _ = ctx.verify_same_message([(msg, keys, sigs)], seed=SEED)
    assert [int(x) for x in got[0]] == [1, 1, -E_BAD, 1, 0, 1]


# ---- bls_gpu_verify_deposits -------------------------------------------------------------------
def _deposit_root(pk: bytes, wc: bytes, amount: int) -> bytes:
    return ssz_oracle.compute_signing_root(ssz_oracle.deposit_message_root(pk, wc, amount), DOMAIN)


@functools.lru_cache(maxsize=None)
def _alias_deposits():
    """(case a, case b) as (pubkey, wc, amount, signature, valid signature): (a) key 1's
    deposit under the alias of its own valid signature -- the first amount whose signature has
    an alias; (b) a deposit whose pubkey FIELD is the alias of key K, its root computed over
    those alias bytes and signed with K's secret key: a decoder that reduces x mod p sees K
    and a valid signature."""
    from oracle import bls_oracle as O

    sk1 = O.interop_secret_key(1)
    pk1, wc = O.g1_compress(O.sk_to_pk(sk1)), _h(b"wire-edge wc")
    for t in range(W.SEARCH):
        amount = 32 * 10**9 + t
        pt = O.sign(sk1, _deposit_root(pk1, wc, amount))
        coord = 0 if pt[0][0] + W.P < W.T381 else 1 if pt[0][1] + W.P < W.T381 else None
        if coord is not None:
            sig = O.g2_compress(pt)
            a = (pk1, wc, amount, W.alias_of(sig, coord), sig)
            break
    else:
        raise AssertionError("no deposit signature with an alias")
    _, sk_k, _ = W.alias_key()
    alias_pk = W.by_name(W.g1_compressed_vectors())["alias"].data
    amount = 32 * 10**9
    sig = O.g2_compress(O.sign(sk_k, _deposit_root(alias_pk, wc, amount)))
    return a, (alias_pk, wc, amount, sig, sig)


def test_verify_deposits_aliases(ctx, oracle):
    a, b = _alias_deposits()
    assert W._sig_vcode(a[3]) == E_BAD and W._sig_vcode(a[4]) == E_OK and oracle.key_validate(a[0]) == E_OK
    assert oracle.key_validate(b[0]) == E_BAD and W._sig_vcode(b[3]) == E_OK
    valid = []
    for k in (2, 3, 4):
        pk, wc, amount = oracle.g1_compress(oracle.sk_to_pk(oracle.interop_secret_key(k))), _h(b"wc%d" % k), 10**9 + k
        sig = ctx.sign(_sk(oracle, k), _deposit_root(pk, wc, amount))[0].tobytes()
        valid.append((pk, wc, amount, sig))
    deps = [valid[0], a[:4], valid[1], b[:4], valid[2], a[:3] + (a[4],)]
    want = [1, -E_BAD, 1, -E_BAD, 1, 1]
    for flags in PATHS.values():
        with _forced(ctx, flags):
            rc, got, _ = ctx.verify_deposits_packed(pack_deposits(deps, DOMAIN, SEED))
        assert rc == 0
        assert [int(x) for x in got] == want, "valid, alias signature, valid, alias pubkey field, valid, (a) unaliased"


# ---- bls_gpu_validate_pubkeys, bls_gpu_load_pubkeys ------------------------------------------------
@pytest.mark.parametrize("pk_len", [48, 96])
def test_validate_pubkeys(gpu, pk_len):
    vecs = W.g1_compressed_vectors() if pk_len == 48 else W.g1_uncompressed_vectors()
    codes = gpu.validate_pubkeys(b"".join(v.data for v in vecs), pk_len)
    for v, code in zip(vecs, codes):
        assert int(code) == v.vcode, "%s (%d bytes): code %d, oracle %d" % (v.name, pk_len, code, v.vcode)


def _table_size(c) -> int:
    return int(c.lib.bls_gpu_load_pubkeys(c._h, None, 0, 48, None))


@pytest.mark.parametrize("pk_len", [48, 96])
def test_load_pubkeys(oracle, pk_len):
    vecs = W.g1_compressed_vectors() if pk_len == 48 else W.g1_uncompressed_vectors()
    with GpuContext(0) as c:
        # the whole list in one call: per-key decode codes; all or nothing, so nothing is appended
        codes = c.load_pubkeys(b"".join(v.data for v in vecs), pk_len)
        for v, code in zip(vecs, codes):
            assert int(code) == v.code, "%s (%d bytes): code %d, oracle %d" % (v.name, pk_len, code, v.code)
        assert _table_size(c) == 0
        # the keys that decode to a finite point: the table holds the oracle's point
        good = [v for v in vecs if v.code == E_OK and v.point is not None]
        assert len(good) >= 2
        assert (c.load_pubkeys(b"".join(v.data for v in good), pk_len) == 0).all()
        assert _table_size(c) == len(good)
        out, codes = c.aggregate_pubkeys([[i] for i in range(len(good))])
        assert (codes == 0).all()
        for v, o in zip(good, out):
            assert o == g1b(v.point), "%s (%d bytes): table point %s" % (v.name, pk_len, o.hex())
        by = {v.name: o for v, o in zip(good, out)}
        a, b = ("canon", "sort_flip") if pk_len == 48 else ("canon", "neg")
        flag = [oracle.g1_compress(oracle.g1_deserialize(by[nm])[1])[0] & 0x20 for nm in (a, b)]
        assert by[a][:48] == by[b][:48] and flag[0] != flag[1]


# ---- raw 96-byte keys in a batch ---------------------------------------------------------------------
def test_verify_raw_pubkey_alias(gpu, oracle):
    """tests/test_gpu_parity.py test_verify_raw_pubkeys with (x + p, y) in the last request:
    a raw key that does not decode rejects every request of the call"""
    u = W.by_name(W.g1_uncompressed_vectors())
    ki, sk_k, _ = W.alias_key()
    assert u["alias_x"].code == E_BAD and u["canon"].vcode == E_OK
    keys = [5, 6, 7]
    msgs = [_h(b"wire-raw%d" % i) for i in range(4)]
    sks = [_sk(oracle, k) for k in keys] + [sk_k.to_bytes(32, "big")]
    sigs = [s.tobytes() for s in gpu.sign(b"".join(sks), b"".join(msgs))]
    raw = [oracle.g1_serialize(oracle.sk_to_pk(oracle.interop_secret_key(k))) for k in keys]
    sets = [(raw[i], msgs[i], sigs[i]) for i in range(3)]
    good = [(False, sets), (True, sets[:1]), (True, sets[1:]), (False, [(u["canon"].data, msgs[3], sigs[3])])]
    v, _ = gpu.verify_packed(pack_requests(good, seed=SEED))
    assert [int(x) for x in v] == [1, 1, 1, 1]
    bad = good[:3] + [(False, [(u["alias_x"].data, msgs[3], sigs[3])])]
    want, _, _ = oracle.verify_many_signature_sets(bad)
    assert [r[0] for r in want] == ["error"] * 4
    v, _ = gpu.verify_packed(pack_requests(bad, seed=SEED))
    assert [int(x) for x in v] == [-r[1].code for r in want] == [-E_BAD] * 4


# ---- bls_gpu_sk_to_pk, bls_gpu_sign at the scalar edges ---------------------------------------------
EDGE_SKS = (("0", 0), ("1", 1), ("r-1", R_ORDER - 1), ("r", R_ORDER), ("r+1", R_ORDER + 1), ("2^256-1", (1 << 256) - 1))


def test_sk_to_pk_and_sign_at_scalar_edges(gpu, oracle):
    assert oracle.R == R_ORDER
    msg = _h(b"wire-edge scalar")
    sks = b"".join(sk.to_bytes(32, "big") for _, sk in EDGE_SKS)
    pks = gpu.sk_to_pk(sks)
    sigs = gpu.sign(sks, msg * len(EDGE_SKS))
    for (nm, sk), pk, sig in zip(EDGE_SKS, pks, sigs):
        want_pk = oracle.g1_compress(oracle.sk_to_pk(sk % R_ORDER))
        want_sig = oracle.g2_compress(oracle.sign(sk % R_ORDER, msg))
        if sk % R_ORDER == 0:
            assert want_pk == bytes([0xC0]) + bytes(47) and want_sig == INF_SIG96
        assert pk.tobytes() == want_pk, "sk = %s: pk %s, want %s" % (nm, pk.tobytes().hex(), want_pk.hex())
        assert sig.tobytes() == want_sig, "sk = %s: signature %s, want %s" % (nm, sig.tobytes().hex(), want_sig.hex())
