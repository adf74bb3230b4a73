"""The addon's verifyDeposits and GpuBlsVerifier.verifyDeposits under Node
(integration/js/depositTest.js): KAT-1 and a 20-deposit mixed list against the verdicts
the Python binding computes on the same GPU; an invalid deposit resolves false."""
from __future__ import annotations

import hashlib
import json
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
ADDON = ROOT / "lodestar_amd" / "_native" / "lodestar_bls.node"
NODE = shutil.which("node")
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

pytestmark = pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or the N-API addon is absent")


def test_addon_exports_verify_deposits():
    code = "const a = require(process.argv[1]); console.log(typeof a.verifyDeposits)"
    out = subprocess.run([NODE, "-e", code, str(ADDON)], capture_output=True, text=True, timeout=60, check=True)
    assert out.stdout.strip() == "function"


def test_js_deposit_domain_and_packer():
    """the domain computed with Node's crypto and the SoA packer, without a GPU"""
    from lodestar_amd.deposits import deposit_domain

    code = ("const m = require(process.argv[1]);"
            "const p = m.packDeposits([{pubkey: Buffer.alloc(48, 1), withdrawalCredentials: Buffer.alloc(32, 2),"
            " amount: 32000000000n, signature: Buffer.alloc(96, 3)}], Buffer.alloc(32, 4));"
            "let bad = 'none'; try { m.packDeposits([{pubkey: Buffer.alloc(48), withdrawalCredentials: "
            "Buffer.alloc(32), amount: 1n << 64n, signature: Buffer.alloc(96)}], Buffer.alloc(32)); }"
            " catch (e) { bad = e.message; }"
            "console.log(JSON.stringify({d: m.depositDomain(Buffer.from('00000001', 'hex')).toString('hex'),"
            " amounts: p.amounts.toString('hex'), n: p.pubkeys.length / 48, bad, cap: m.DEPOSITS_MAX_CALL}))")
    out = subprocess.run([NODE, "-e", code, str(ROOT / "integration" / "js" / "gpuBlsVerifier.js")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["d"] == deposit_domain(bytes.fromhex("00000001")).hex()
    assert r["amounts"] == (32 * 10**9).to_bytes(8, "little").hex() and r["n"] == 1
    assert "uint64" in r["bad"] and r["cap"] == 65536


@pytest.mark.gpu
def test_js_verify_deposits(gpu, golden, tmp_path):
    from lodestar_amd._abi import SSZ_DEPOSIT_MESSAGE
    from lodestar_amd.deposits import deposit_domain, verify_deposit_codes

    fork_version = bytes.fromhex("00000001")
    domain = deposit_domain(fork_version)
    kat = json.loads((ROOT / "tests" / "golden" / "ssz_golden.json").read_text())["kat1_deposit"]
    kat1 = (bytes.fromhex(kat["pubkey"]), bytes.fromhex(kat["withdrawal_credentials"]), kat["amount"],
            bytes.fromhex(golden["kat1"]["signature"]))
    n = 20
    sks = [int.from_bytes(hashlib.sha256(b"napi deposit%d" % i).digest(), "little") % R_ORDER for i in range(n)]
    sk_bytes = b"".join(s.to_bytes(32, "big") for s in sks)
    pks = [p.tobytes() for p in gpu.sk_to_pk(sk_bytes)]
    fields = [(pks[i], hashlib.sha256(b"wc%d" % i).digest(), 32 * 10**9 + i) for i in range(n)]
    objs = b"".join(pk + wc + a.to_bytes(8, "little") for pk, wc, a in fields)
    roots = gpu.ssz_roots(SSZ_DEPOSIT_MESSAGE, objs, domain)
    sigs = [s.tobytes() for s in gpu.sign(sk_bytes, roots.tobytes())]
    deps = [list(f) + [s] for f, s in zip(fields, sigs)]
    deps[0][2] += 1                                   # amount off by one
    deps[3][0] = bytes([0xC0]) + bytes(47)            # the infinity key
    deps[7][3] = sigs[8]                              # another key's signature
    deps[12][3] = bytes([0xC0]) + bytes(95)           # the infinity signature
    deps[16][0] = bytes([pks[16][0] & 0x7F]) + pks[16][1:]  # compression flag cleared
    deps[19][1] = bytes(32)                           # other withdrawal credentials
    codes = [int(c) for c in verify_deposit_codes(gpu, [tuple(d) for d in deps], domain=domain)]
    bad = (0, 3, 7, 12, 16, 19)
    assert [c == 1 for c in codes] == [k not in bad for k in range(n)]
    assert [int(c) for c in verify_deposit_codes(gpu, [kat1], fork_version=fork_version)] == [1]

    def js(d):
        return {"pubkey": d[0].hex(), "wc": d[1].hex(), "amount": str(d[2]), "signature": d[3].hex()}

    f = tmp_path / "deposits.json"
    f.write_text(json.dumps({"forkVersion": fork_version.hex(), "domain": domain.hex(), "kat1": js(kat1),
                             "deposits": [js(d) for d in deps]}))
    out = subprocess.run([NODE, str(ROOT / "integration" / "js" / "depositTest.js"), str(f)], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["addon"] == "function" and r["domain"] == domain.hex()
    assert r["kat1"] == [True] and r["kat1Tampered"] == [False]
    assert r["mixed"] == [c == 1 for c in codes] == r["mixedByDomain"]
    assert r["native"]["verdicts"] == codes and r["native"]["nChunks"] == 1
    assert r["empty"] == [] and r["shortSignature"] == [True, False]
    assert "forkVersion or domain" in r["noDomain"]
