"""bls_gpu_verify_deposits without a GPU: the front kernel's per-item stages
(lodestar_amd/csrc/bls/deposit.hpp) compiled for the host and run by the stand-alone
program tests/native/deposit_host.cpp, against the oracle; the binding, the packer, the
domain and the split at the call cap."""
from __future__ import annotations

import ctypes
import json
import subprocess
from pathlib import Path

import pytest

from lodestar_amd import _abi
from lodestar_amd._abi import BlsDepositBatch, BlsStats, load_library
from lodestar_amd.build import build_deposit_host
from lodestar_amd.deposits import deposit_domain, screen_deposits, split_deposits
from lodestar_amd.native import pack_deposits
from oracle import ssz_oracle
from tests._groupedge import low_order_keys, neg_compressed

ROOT = Path(__file__).resolve().parent.parent
SSZ_GOLDEN = json.loads((ROOT / "tests" / "golden" / "ssz_golden.json").read_text())
KAT1 = SSZ_GOLDEN["kat1_deposit"]
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
INF96 = bytes([0x40]) + bytes(95)


def _run(exe: Path, records: list[str]) -> list[list[str]]:
    out = subprocess.run([str(exe)], input="\n".join(records) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln.split() for ln in out.stdout.splitlines()]
    assert len(lines) == len(records)
    return lines


@pytest.fixture(scope="module")
def host():
    return build_deposit_host(verbose=False)


def _x_key(x: int, sort_bit: int = 0) -> bytes:
    """the compressed encoding of abscissa x (any 381-bit value), compression flag set"""
    b = bytearray(x.to_bytes(48, "big"))
    assert b[0] < 0x20
    b[0] |= 0x80 | (0x20 if sort_bit else 0)
    return bytes(b)


@pytest.fixture(scope="module")
def key_cases(golden, oracle):
    """[(name, 48 bytes)]: the key list of the issue (shared with the GPU tests' bad keys)"""
    interop = [bytes.fromhex(h) for h in golden["kat2_interop_pubkeys"][:10]]
    cases = [("interop%d" % k, pk) for k, pk in enumerate(interop)]
    cases += [
        ("infinity", bytes([0xC0]) + bytes(47)),
        ("infinity_stray_bit", bytes([0xC0]) + bytes(46) + b"\x01"),
        ("no_compression_flag", bytes([interop[0][0] & 0x7F]) + interop[0][1:]),
        ("x_eq_p", _x_key(P)),
        ("x_eq_p_minus_1", _x_key(P - 1)),
        ("x_eq_1", _x_key(1)),
    ]
    cases += [(name, oracle.g1_compress(pt)) for name, pt in low_order_keys()]
    cases.append(("sign_flipped", neg_compressed(interop[3])))
    return cases


def _root_record(pk: bytes, wc: bytes, amount: int, domain: bytes) -> str:
    return "root %s %s %s %s" % (pk.hex(), wc.hex(), amount.to_bytes(8, "little").hex(), domain.hex())


def _oracle_root(pk: bytes, wc: bytes, amount: int, domain: bytes) -> bytes:
    return ssz_oracle.compute_signing_root(ssz_oracle.deposit_message_root(pk, wc, amount), domain)


ROOT_CASES = [
    (bytes.fromhex(KAT1["pubkey"]), bytes.fromhex(KAT1["withdrawal_credentials"]), a, bytes.fromhex(KAT1["domain"]))
    for a in (KAT1["amount"], 0, 1, 32 * 10**9, 2**64 - 1)
] + [(b"\xff" * 48, b"\xff" * 32, 32 * 10**9, bytes(range(32)))]


def test_signing_roots_match_the_oracle(host):
    got = _run(host, [_root_record(*c) for c in ROOT_CASES])
    for c, ln in zip(ROOT_CASES, got):
        assert ln == ["root", _oracle_root(*c).hex()], c[2]
    # KAT-1: the root the reference's genesis test signs (genesisState.test.ts:65-69)
    assert got[0][1] == KAT1["signing_root"]


def test_deposit_domain():
    assert deposit_domain(bytes.fromhex("00000001")) == bytes.fromhex(KAT1["domain"])
    assert deposit_domain(bytes.fromhex(KAT1["fork_version"]), bytes.fromhex(KAT1["genesis_validators_root"])) == \
        ssz_oracle.compute_domain(bytes.fromhex("03000000"), bytes.fromhex("00000001"), bytes(32))
    with pytest.raises(ValueError):
        deposit_domain(b"\0" * 3)


def test_key_stage_matches_the_oracle(host, key_cases, oracle):
    got = _run(host, ["key " + pk.hex() for _, pk in key_cases])
    codes = {}
    for (name, pk), ln in zip(key_cases, got):
        code, pt = oracle.g1_decompress(pk)
        want = oracle.key_validate(pk)
        codes[name] = want
        assert ln[0] == "key" and int(ln[1]) == want, (name, ln[1], want)
        # the decoded point (the infinity encoding when the bytes do not decode)
        assert bytes.fromhex(ln[2]) == (oracle.g1_serialize(pt) if code == 0 else INF96), name
        # only a validated key is handed on to the verify pass
        assert int(ln[3]) == (1 if want == 0 else 0), name
    # what the oracle gives today for the edge encodings
    assert [codes["interop%d" % k] for k in range(10)] == [0] * 10
    assert codes["infinity"] == 6
    assert codes["infinity_stray_bit"] == codes["no_compression_flag"] == codes["x_eq_p"] == 1
    assert codes["x_eq_1"] == 2
    assert [codes[name] for name, _ in low_order_keys()] == [3] * 6
    assert codes["sign_flipped"] == 0


def test_sign_flipped_key_is_the_negation(host, golden, oracle):
    pk = bytes.fromhex(golden["kat2_interop_pubkeys"][3])
    a, b = _run(host, ["key " + pk.hex(), "key " + neg_compressed(pk).hex()])
    pa, pb = bytes.fromhex(a[2]), bytes.fromhex(b[2])
    assert pa[:48] == pb[:48]
    assert (int.from_bytes(pa[48:], "big") + int.from_bytes(pb[48:], "big")) == P


def test_deposit_call_plan(host):
    """a deposit call as n one-set batchable requests: the chunks are those of
    chunkifyMaximizeChunkSize(n, 16), the cap and the NULL checks refuse with -2"""
    from lodestar_amd.verifier import chunkify_maximize_chunk_size

    sizes = [0, 1, 15, 16, 17, 31, 32, 33, 65, 129, 1000, _abi.DEPOSITS_MAX_CALL]
    got = _run(host, ["plan %d" % n for n in sizes + [_abi.DEPOSITS_MAX_CALL + 1]])
    for n, ln in zip(sizes, got):
        chunks = [len(c) for c in chunkify_maximize_chunk_size(list(range(n)), 16)] if n else []
        want = ",".join(str(c) for c in chunks) if chunks else "-"
        assert ln == ["plan", str(n), "0", str(len(chunks)), want], n
    assert got[-1] == ["plan", str(_abi.DEPOSITS_MAX_CALL + 1), "-2", "0", "-"]


def test_malformed_record_is_refused(host):
    out = subprocess.run([str(host)], input="key 00\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "malformed" in out.stderr


def test_stages_under_sanitizers(tmp_path, key_cases):
    """the same stand-alone program compiled with -fsanitize=address,undefined, run once
    over every record of this file: any report makes it exit non-zero"""
    exe = build_deposit_host(verbose=False, out=tmp_path / "deposit_host_san",
                             extra=["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                    "-fno-omit-frame-pointer"])
    recs = [_root_record(*c) for c in ROOT_CASES] + ["key " + pk.hex() for _, pk in key_cases]
    recs += ["plan %d" % n for n in (0, 1, 17, 65, 4096, _abi.DEPOSITS_MAX_CALL, _abi.DEPOSITS_MAX_CALL + 1)]
    f = tmp_path / "records.txt"
    f.write_text("\n".join(recs) + "\n")
    out = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-4000:]
    assert out.stdout == "".join(" ".join(ln) + "\n" for ln in _run(build_deposit_host(verbose=False), recs))


# -- the binding and the packer ---------------------------------------------------
def test_binding_exists_and_refuses_bad_arguments_without_a_device():
    lib = load_library()
    assert lib.bls_gpu_verify_deposits.restype is ctypes.c_int
    b = BlsDepositBatch()
    b.n = 3
    st = BlsStats()
    # no context: refused before anything is read
    assert lib.bls_gpu_verify_deposits(None, ctypes.byref(b), None, ctypes.byref(st)) == -2
    assert [f for f, _ in BlsDepositBatch._fields_] == ["n", "pubkeys48", "withdrawal_credentials", "amounts",
                                                         "signatures", "domain", "seed"]
    hdr = (ROOT / "include" / "lodestar_bls.h").read_text()
    assert "#define BLS_DEPOSITS_MAX_CALL %du" % _abi.DEPOSITS_MAX_CALL in hdr


def _dep(k: int = 0, amount: int = 32 * 10**9):
    return (bytes([0x80 + k % 16]) + bytes(47), bytes([k % 256]) * 32, amount, bytes([0xA0]) + bytes([k % 256]) * 95)


def test_pack_deposits_layout():
    deps = [_dep(k, amount=k * 1000 + 1) for k in range(5)]
    pd = pack_deposits(deps, bytes(range(32)), seed=b"\x07" * 32)
    assert pd.n == 5 and pd.seed == b"\x07" * 32
    assert pd.pubkeys48.tobytes() == b"".join(d[0] for d in deps)
    assert pd.withdrawal_credentials.tobytes() == b"".join(d[1] for d in deps)
    assert pd.amounts.tobytes() == b"".join(d[2].to_bytes(8, "little") for d in deps)
    assert pd.signatures.tobytes() == b"".join(d[3] for d in deps)
    assert pd.domain.tobytes() == bytes(range(32))
    assert pack_deposits([], bytes(32)).n == 0


@pytest.mark.parametrize("bad", [
    (b"\x80" * 47, bytes(32), 1, bytes(96)),
    (b"\x80" * 96, bytes(32), 1, bytes(96)),
    (b"\x80" * 48, bytes(31), 1, bytes(96)),
    (b"\x80" * 48, bytes(32), 1, bytes(95)),
    (b"\x80" * 48, bytes(32), -1, bytes(96)),
    (b"\x80" * 48, bytes(32), 2**64, bytes(96)),
])
def test_pack_deposits_refuses_bad_fields(bad):
    with pytest.raises(ValueError):
        pack_deposits([_dep(0), bad], bytes(32))


def test_pack_deposits_refuses_a_bad_domain():
    with pytest.raises(ValueError):
        pack_deposits([_dep(0)], bytes(31))
    assert pack_deposits([_dep(0, 2**64 - 1)], bytes(32)).amounts.tobytes() == b"\xff" * 8


def test_split_at_the_cap(monkeypatch):
    deps = [_dep(k) for k in range(11)]
    assert split_deposits(deps) == [deps]  # far below BLS_DEPOSITS_MAX_CALL
    monkeypatch.setattr(_abi, "DEPOSITS_MAX_CALL", 4)
    parts = split_deposits(deps)
    assert [len(p) for p in parts] == [4, 4, 3]
    assert [d for p in parts for d in p] == deps
    assert [len(p) for p in split_deposits(deps[:8])] == [4, 4]
    assert split_deposits([]) == []


def test_wrong_length_signature_is_screened_not_raised():
    deps = [_dep(0), _dep(1)[:3] + (bytes(95),), _dep(2), _dep(3)[:3] + (b"",)]
    taken, pos = screen_deposits(deps)
    assert pos == [0, 2] and taken == [deps[0], deps[2]]
