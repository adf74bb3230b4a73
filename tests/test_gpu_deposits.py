"""bls_gpu_verify_deposits on cuda:0 (processDeposit.ts:48-65).

Expected verdicts come from: the reference's own known answer (KAT-1, the interop deposit
of genesisState.test.ts:65-69); by construction (a deposit signed with its own key over its
own fields is valid); oracle.key_validate for the key codes; bls_gpu_verify over the same
sets with the keys in a second context's table and the roots from bls_gpu_ssz_roots (the
existing, oracle-checked path) for everything else; and oracle.core_verify for three of
the zero verdicts.  Every comparison is exact."""
from __future__ import annotations

import ctypes
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from lodestar_amd import _abi
from lodestar_amd._abi import (
    CODE_BAD_ENCODING,
    CODE_INVALID_SIZE,
    CODE_POINT_NOT_IN_GROUP,
    CODE_ZERO_SIGNATURE,
    DEBUG_FORCE_EXACT,
    DEBUG_MSM,
    DEBUG_SIGAGG_OFF,
    DEBUG_SIGAGG_ON,
    SSZ_DEPOSIT_MESSAGE,
)
from lodestar_amd.deposits import deposit_domain, verify_deposit_codes, verify_deposits
from lodestar_amd.native import GpuContext, PackedDeposits, pack_deposits, pack_requests
from tests._groupedge import low_order_keys, low_order_sigs, neg_compressed

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KAT1 = json.loads((ROOT / "tests" / "golden" / "ssz_golden.json").read_text())["kat1_deposit"]
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
N = 129
SHAPES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)  # chunkify(.., 16) and wavefront edges
SEED = bytes(range(32))
FORK_VERSION = bytes.fromhex("00000001")
DOMAIN = deposit_domain(FORK_VERSION)
OTHER_DOMAIN = deposit_domain(bytes.fromhex("00000002"))
STAT_FIELDS = ("batch_retries", "batch_sigs_success", "n_chunks", "n_individual", "n_flagged", "n_unique_msgs",
               "merged_check", "n_ml_units", "pass_shape")


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def _x_key(x: int) -> bytes:
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80
    return bytes(b)


class _Fixture:
    """N valid deposits, key i signing its own DepositMessage; a second context whose table
    holds the N keys is the reference (bls_gpu_verify over table indices)."""

    def __init__(self):
        self.ctx = GpuContext(0)
        self.ref = GpuContext(0)
        self.sks = [int.from_bytes(_h(b"deposit sk" + i.to_bytes(4, "little")), "little") % R_ORDER for i in range(N)]
        pks = self.ctx.sk_to_pk(b"".join(s.to_bytes(32, "big") for s in self.sks))
        self.pks = [p.tobytes() for p in pks]
        assert (self.ref.load_pubkeys(b"".join(self.pks), 48) == 0).all()
        fields = [(self.pks[i], _h(b"wc" + bytes([i])), 32 * 10**9 + i) for i in range(N)]
        sigs = self.sign(range(N), self.roots(fields))
        self.deposits = tuple((pk, wc, amount, sig) for (pk, wc, amount), sig in zip(fields, sigs))

    def close(self):
        self.ctx.close()
        self.ref.close()

    def roots(self, fields, domain: bytes = DOMAIN) -> list[bytes]:
        """signing roots of (pubkey, wc, amount, ...) tuples by bls_gpu_ssz_roots"""
        objs = b"".join(bytes(f[0]) + bytes(f[1]) + int(f[2]).to_bytes(8, "little") for f in fields)
        return [r.tobytes() for r in self.ctx.ssz_roots(SSZ_DEPOSIT_MESSAGE, objs, domain)]

    def sign(self, indices, roots) -> list[bytes]:
        out = self.ctx.sign(b"".join(self.sks[i].to_bytes(32, "big") for i in indices), b"".join(roots))
        return [s.tobytes() for s in out]

    def call(self, deposits, seed=SEED, flags: int = 0, ctx=None):
        ctx = ctx or self.ctx
        ctx.set_debug_flags(flags)
        try:
            rc, v, st = ctx.verify_deposits_packed(pack_deposits(deposits, DOMAIN, seed))
        finally:
            ctx.set_debug_flags(0)
        assert rc == 0, ctx.lib.bls_gpu_last_error(ctx._h)
        return [int(x) for x in v], st

    def reference(self, deposits, key_indices, batchable: bool, seed=SEED):
        """bls_gpu_verify over one-set requests (table key key_indices[k], the root of
        deposit k's own fields, its signature) on the second context"""
        roots = self.roots(deposits)
        reqs = [(batchable, [([i], r, d[3])]) for i, r, d in zip(key_indices, roots, deposits)]
        v, st = self.ref.verify_packed(pack_requests(reqs, seed=seed))
        return [int(x) for x in v], st


@pytest.fixture(scope="module")
def dp():
    f = _Fixture()
    yield f
    f.close()


def test_kat1(dp, golden):
    dep = (bytes.fromhex(KAT1["pubkey"]), bytes.fromhex(KAT1["withdrawal_credentials"]), KAT1["amount"],
           bytes.fromhex(golden["kat1"]["signature"]))
    assert dp.call([dep])[0] == [1]
    assert dp.call([dep[:2] + (dep[2] + 1,) + dep[3:]])[0] == [0]
    assert verify_deposits(dp.ctx, [dep], FORK_VERSION) == [True]


@pytest.mark.parametrize("n", SHAPES)
def test_shapes_all_valid(dp, n):
    deps = list(dp.deposits[:n])
    flag_sets = [0, DEBUG_SIGAGG_OFF, DEBUG_SIGAGG_ON] + ([DEBUG_FORCE_EXACT] if n <= 17 else [])
    plain = None
    for flags in flag_sets:
        v, st = dp.call(deps, flags=flags)
        assert v == [1] * n, (flags, v)
        assert st.n_unique_msgs == n
        if flags == 0:
            plain = st
    # the stats of bls_gpu_verify over the same sets as one-set batchable requests
    v, ref = dp.reference(deps, range(n), batchable=True)
    assert v == [1] * n
    for f in STAT_FIELDS:
        assert getattr(plain, f) == getattr(ref, f), f


@pytest.fixture(scope="module")
def bad_keys(golden, oracle):
    """the keys of tests/test_deposits_cpu.py that are no valid key: [(name, 48 bytes)]"""
    k0 = bytes.fromhex(golden["kat2_interop_pubkeys"][0])
    keys = [
        ("infinity", bytes([0xC0]) + bytes(47)),
        ("infinity_stray_bit", bytes([0xC0]) + bytes(46) + b"\x01"),
        ("no_compression_flag", bytes([k0[0] & 0x7F]) + k0[1:]),
        ("x_eq_p", _x_key(P)),
        ("x_eq_p_minus_1", _x_key(P - 1)),
        ("x_eq_1", _x_key(1)),
    ]
    keys += [(name, oracle.g1_compress(pt)) for name, pt in low_order_keys()]
    return [(name, pk) for name, pk in keys if oracle.key_validate(pk) != 0]


# positions of the 65-deposit mixed call: chunks of chunkify(65, 16) are [0, 17), [17, 34),
# [34, 51), [51, 65)
MIXED_N = 65
AMOUNT, WRONG_WC, OTHER_KEY, OTHER_DOMAIN_AT, NEGATED, INF_SIG, ORDER13 = 0, 16, 17, 30, 33, 40, 50
X_GE_P, FLIPPED_KEY = 64, 62
KEY_AT = (2, 5, 20, 22, 25, 36, 38, 42, 45, 52, 55, 60)


@pytest.fixture(scope="module")
def mixed(dp, bad_keys):
    """(the 65 deposits, {position of a bad key: its name in bad_keys})"""
    d = [list(x) for x in dp.deposits[:MIXED_N]]
    d[AMOUNT][2] += 1
    d[WRONG_WC][1] = _h(b"another wc")
    d[OTHER_KEY][3] = dp.deposits[OTHER_KEY + 1][3]
    d[OTHER_DOMAIN_AT][3] = dp.sign([OTHER_DOMAIN_AT], dp.roots([d[OTHER_DOMAIN_AT]], OTHER_DOMAIN))[0]
    d[NEGATED][3] = neg_compressed(d[NEGATED][3])
    d[INF_SIG][3] = bytes([0xC0]) + bytes(95)
    d[ORDER13][3] = low_order_sigs()[0][0]
    d[X_GE_P][3] = bytes([0x9F]) + b"\xff" * 95
    # a valid key (the negation of key 62) under key 62's signature
    d[FLIPPED_KEY][0] = neg_compressed(d[FLIPPED_KEY][0])
    assert len(bad_keys) <= len(KEY_AT)
    key_pos = {}
    for at, (name, pk) in zip(KEY_AT, bad_keys):
        d[at][0] = pk  # the signature stays: valid for key `at`, over the original fields
        key_pos[at] = name
    return [tuple(x) for x in d], key_pos


@pytest.mark.parametrize("flags", [DEBUG_SIGAGG_OFF, DEBUG_SIGAGG_ON])
def test_mixed_call(dp, mixed, bad_keys, oracle, flags):
    deps, key_pos = mixed
    v, st = dp.call(deps, flags=flags)
    # key codes: the oracle's KeyValidate
    names = dict(bad_keys)
    for at, name in key_pos.items():
        assert v[at] == -oracle.key_validate(names[name]), (name, v[at])
    # everything else: the reference call, non-batchable one-set requests over table keys
    others = [k for k in range(MIXED_N) if k not in key_pos and k != FLIPPED_KEY]
    ref, _ = dp.reference([deps[k] for k in others], others, batchable=False)
    assert [v[k] for k in others] == ref
    assert v[INF_SIG] == -CODE_ZERO_SIGNATURE and v[ORDER13] == -CODE_POINT_NOT_IN_GROUP
    assert v[X_GE_P] == -CODE_BAD_ENCODING
    assert [v[k] for k in (AMOUNT, WRONG_WC, OTHER_KEY, OTHER_DOMAIN_AT, NEGATED, FLIPPED_KEY)] == [0] * 6
    # isolation: every untouched deposit is valid
    touched = set(key_pos) | {AMOUNT, WRONG_WC, OTHER_KEY, OTHER_DOMAIN_AT, NEGATED, INF_SIG, ORDER13, X_GE_P,
                              FLIPPED_KEY}
    assert [v[k] for k in range(MIXED_N) if k not in touched] == [1] * (MIXED_N - len(touched))
    assert st.n_chunks == 4 and st.n_unique_msgs == MIXED_N


def test_mixed_zero_verdicts_against_the_oracle(dp, mixed, oracle):
    deps, _ = mixed
    roots = dp.roots(deps)
    for k in (AMOUNT, OTHER_KEY, NEGATED):
        code, pk = oracle.g1_decompress(deps[k][0])
        assert code == 0
        assert oracle.core_verify(pk, roots[k], deps[k][3]) is False


def test_duplicates(dp):
    """the same valid deposit four times in one call: equal points meet in the signature sums"""
    deps = list(dp.deposits[:64])
    for at in (3, 19, 35, 63):
        deps[at] = dp.deposits[7]
    for flags in (0, DEBUG_SIGAGG_ON, DEBUG_SIGAGG_ON | DEBUG_MSM):
        v, st = dp.call(deps, flags=flags)
        assert v == [1] * 64, flags
        assert st.n_unique_msgs == 64  # no signing-root dedup


def test_determinism(dp, mixed):
    deps, _ = mixed
    a, _ = dp.call(deps, seed=SEED)
    b, _ = dp.call(deps, seed=_h(b"another seed"))
    c, _ = dp.call(deps, seed=None)
    assert a == b == c


def _table_size(ctx) -> int:
    return int(ctx.lib.bls_gpu_load_pubkeys(ctx._h, None, 0, 48, None))  # appends nothing


def test_table_untouched(dp, mixed):
    deps, _ = mixed
    ctx = dp.ref  # its table holds the N keys
    reqs = [(True, [([i], r, d[3])]) for i, (r, d) in enumerate(zip(dp.roots(dp.deposits[:20]), dp.deposits[:20]))]
    reqs[5] = (True, [([6], reqs[5][1][0][1], reqs[5][1][0][2])])
    pb = pack_requests(reqs, seed=SEED)
    size = _table_size(ctx)
    assert size == N
    before, _ = ctx.verify_packed(pb)
    v, _ = dp.call(deps, ctx=ctx)
    assert v == dp.call(deps)[0]
    assert _table_size(ctx) == size
    after, _ = ctx.verify_packed(pb)
    assert list(before) == list(after) == [1] * 5 + [0] + [1] * 14


def test_merged_check_history_is_left_alone(dp):
    ctx = dp.ref
    reqs = [(True, [([i], r, d[3])]) for i, (r, d) in enumerate(zip(dp.roots(dp.deposits[:40]), dp.deposits[:40]))]
    pb = pack_requests(reqs, seed=SEED)
    ctx.verify_packed(pb)  # (whatever ran on this context before, a passing pass clears its history)
    v, st = ctx.verify_packed(pb)
    assert list(v) == [1] * 40 and st.merged_check == 1
    deps = list(dp.deposits[:40])
    deps[9] = deps[9][:2] + (deps[9][2] + 1,) + deps[9][3:]
    v, st = dp.call(deps, ctx=ctx)
    assert v == [1] * 9 + [0] + [1] * 30 and st.merged_check == 2  # the deposit call's own check failed
    v, st = ctx.verify_packed(pb)
    assert list(v) == [1] * 40 and st.merged_check == 1  # not 3: the history was not written


def test_arguments(dp):
    rc, v, _ = dp.ctx.verify_deposits_packed(pack_deposits([], DOMAIN))
    assert rc == 0 and len(v) == 0
    n = _abi.DEPOSITS_MAX_CALL + 1
    big = PackedDeposits(pubkeys48=np.zeros(48 * n, np.uint8), withdrawal_credentials=np.zeros(32 * n, np.uint8),
                         amounts=np.zeros(8 * n, np.uint8), signatures=np.zeros(96 * n, np.uint8),
                         domain=np.zeros(32, np.uint8), n=n)
    rc, _, _ = dp.ctx.verify_deposits_packed(big)
    assert rc == -2
    assert b"BLS_DEPOSITS_MAX_CALL" in dp.ctx.lib.bls_gpu_last_error(dp.ctx._h)
    fields = ("pubkeys48", "withdrawal_credentials", "amounts", "signatures", "domain")
    pd = pack_deposits(list(dp.deposits[:3]), DOMAIN)
    out = np.zeros(3, np.int32)
    for missing in fields + ("verdicts",):
        b = _abi.BlsDepositBatch()
        b.n = 3
        for f in fields:
            setattr(b, f, None if f == missing else getattr(pd, f).ctypes.data)
        rc = dp.ctx.lib.bls_gpu_verify_deposits(dp.ctx._h, ctypes.byref(b), None if missing == "verdicts" else
                                                out.ctypes.data, None)
        assert rc == -2, missing
    # the call still works afterwards, without stats too
    assert dp.call(list(dp.deposits[:3]))[0] == [1, 1, 1]


def test_python_helpers(dp):
    deps = list(dp.deposits[:6])
    deps[2] = deps[2][:3] + (deps[2][3][:95],)  # a signature of the wrong length: invalid, no exception
    deps[4] = deps[4][:2] + (1,) + deps[4][3:]
    assert verify_deposits(dp.ctx, deps, FORK_VERSION) == [True, True, False, True, False, True]
    codes = verify_deposit_codes(dp.ctx, deps, domain=DOMAIN, seed=SEED)
    assert list(codes) == [1, 1, -CODE_INVALID_SIZE, 1, 0, 1]
    assert verify_deposits(dp.ctx, [], FORK_VERSION) == []


def test_multi_device(dp, monkeypatch):
    from lodestar_amd.verifier import GpuBlsVerifier

    deps = list(dp.deposits[:40])
    deps[0] = deps[0][:2] + (7,) + deps[0][3:]
    deps[16] = (bytes([0xC0]) + bytes(47),) + deps[16][1:]
    deps[39] = deps[39][:3] + (deps[38][3],)
    single = [x == 1 for x in dp.call(deps)[0]]
    assert single == [k not in (0, 16, 39) for k in range(40)]
    monkeypatch.setattr(_abi, "DEPOSITS_MAX_CALL", 16)
    with GpuBlsVerifier(devices=[0, 0], n_contexts=1) as v:
        got = v.verify_deposits(deps, FORK_VERSION)
        assert got == single and all(isinstance(x, bool) for x in got)
        assert sum(s["calls"] for s in v.slot_stats) == 3 and sum(s["sets"] for s in v.slot_stats) == 40
        assert v.verify_deposits([], FORK_VERSION) == []
