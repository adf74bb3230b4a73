"""One key table per device through the N-API addon (sharePubkeys, pubkeysInfo) and the JS
GpuBlsVerifier's sharePubkeys option under Node (integration/js/sharedTableTest.js): one
table id over the verifier's four contexts, one load, a later loadPubkeys that appends
once, and verdicts; the option off gives a table per context."""
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
N_FIRST, N_LATER = 73, 10

pytestmark = pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or the N-API addon is absent")


def test_addon_exports_the_table_functions():
    code = "const a = require(process.argv[1]); console.log(typeof a.sharePubkeys, typeof a.pubkeysInfo)"
    out = subprocess.run([NODE, "-e", code, str(ADDON)], capture_output=True, text=True, timeout=60, check=True)
    assert out.stdout.split() == ["function", "function"]


@pytest.mark.gpu
def test_js_verifier_shares_one_table(gpu, oracle, tmp_path):
    n = N_FIRST + N_LATER
    sks = [oracle.interop_secret_key(i).to_bytes(32, "big") for i in range(n)]
    pks = gpu.sk_to_pk(b"".join(sks))

    def sets(keys, tag):
        msgs = [hashlib.sha256(tag + b"%d" % i).digest() for i in range(len(keys))]
        sigs = gpu.sign(b"".join(sks[k] for k in keys), b"".join(msgs))
        return [{"idx": k, "msg": m.hex(), "sig": s.tobytes().hex()} for k, m, s in zip(keys, msgs, sigs)]

    sm_msg = hashlib.sha256(b"napi shared same message").digest()
    sm_keys = list(range(40, 60))
    sm_sigs = gpu.sign(b"".join(sks[k] for k in sm_keys), sm_msg * len(sm_keys))
    f = tmp_path / "shared.json"
    f.write_text(json.dumps({
        "first48": pks[:N_FIRST].tobytes().hex(), "later48": pks[N_FIRST:].tobytes().hex(),
        "sets": sets(list(range(0, 40)), b"napi-shared-"), "laterSets": sets(list(range(N_FIRST, n)), b"napi-later-"),
        "smMsg": sm_msg.hex(), "smSets": [{"idx": k, "sig": s.tobytes().hex()} for k, s in zip(sm_keys, sm_sigs)]}))
    out = subprocess.run([NODE, str(ROOT / "integration" / "js" / "sharedTableTest.js"), str(f)], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["addon"] == ["function", "function"] and r["tableCtxs"] == 1
    # one id, one load
    assert r["loadsFirst"] == 1 and len(r["first"]) == 4
    assert len({i["tableId"] for i in r["first"]}) == 1 and r["first"][0]["tableId"] != 0
    cap = 3 * N_FIRST // 2 + 1024
    for i in r["first"]:
        assert (i["nKeys"], i["combKeys"], i["nContexts"], i["capacity"]) == (N_FIRST, N_FIRST, 4, cap)
        assert i["deviceBytes"] == cap * (100 + 1440 + 1)
    # verdicts
    assert r["batchable"] == [True] * 40 and r["mainLane"] is True and r["wrong"] is False
    assert r["sameMessage"] == [True] * len(sm_keys)
    # a later loadPubkeys appends once, for everyone
    assert r["loadsLater"] == 1
    assert [i["nKeys"] for i in r["later"]] == [n] * 4
    assert r["laterPool"] == [True] * N_LATER and r["laterMain"] is True
    assert "batch index 1" in r["badLoad"] and r["afterBad"] == [n] * 4
    # refusals
    assert "holds" in r["refuseHoldsKeys"] and "itself" in r["refuseSelf"] and r["again"] == "shared"
    assert r["loneInfo"]["nKeys"] == 1 and r["loneInfo"]["nContexts"] == 1
    assert r["loneInfo"]["tableId"] != r["first"][0]["tableId"]
    # the option off
    assert len(set(r["ownIds"])) == 4 and r["ownTableCtxs"] is None and r["ownVerdict"] is True
