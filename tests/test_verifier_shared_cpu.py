"""The verifiers' share_pubkeys / sharePubkeys option on the CPU, over stand-in contexts:
with a share method the first context opened on a device owns the table, every other
context there shares it and a load reaches one context per device; `devices=[0, 0]` is one
device; a stand-in without the method (tests/_standin.py's TokenCtx, the JS tests' fake
addons) gets per-context loads as before."""
from __future__ import annotations

import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lodestar_amd.verifier import BlsError, GpuBlsVerifier
from tests._standin import TokenCtx

ROOT = Path(__file__).resolve().parent.parent
NODE = shutil.which("node")


class SharingCtx(TokenCtx):
    """a TokenCtx that has the share method: `table` is the list of loaded batches, shared
    by reference with the contexts that joined it"""

    opened: list = []

    def __init__(self, device, high_priority=False):
        super().__init__(device, high_priority, delay_s=0.0)
        self.table, self.loads, self.shared_with = [], 0, None
        SharingCtx.opened.append(self)

    def share_pubkeys(self, other):
        assert other is not self and other.device == self.device and not self.table
        self.table, self.shared_with = other.table, other

    def load_pubkeys(self, pks, width=48):
        self.loads += 1
        codes = np.array([1 if pks[i:i + width] == b"\xff" * width else 0 for i in range(0, len(pks), width)],
                         dtype=np.int32)
        if not codes.any():
            self.table.append(bytes(pks))
        return codes


def _open(**kw):
    SharingCtx.opened = []
    v = GpuBlsVerifier(context_factory=SharingCtx, **kw)
    return v, list(SharingCtx.opened)


def test_one_load_per_device():
    v, ctxs = _open(devices=[0, 1], n_contexts=2, pubkeys48=b"\x01" * 96)
    try:
        assert ctxs[0].high and [c.device for c in ctxs] == [0, 0, 0, 1, 1]
        owner0, owner1 = ctxs[0], ctxs[3]  # the main-thread lane; device 1's first pool context
        assert [c.shared_with for c in ctxs] == [None, owner0, owner0, None, owner1]
        assert [c.loads for c in ctxs] == [1, 0, 0, 1, 0]
        v.load_pubkeys(b"\x02" * 48)
        assert [c.loads for c in ctxs] == [2, 0, 0, 2, 0]
        assert all(c.table == [b"\x01" * 96, b"\x02" * 48] for c in ctxs)
        assert owner0.table is not owner1.table
        # all or nothing, first device first: the bad batch stops at the first device
        with pytest.raises(BlsError, match="batch index 1"):
            v.load_pubkeys(b"\x03" * 48 + b"\xff" * 48)
        assert [c.loads for c in ctxs] == [3, 0, 0, 2, 0]
        assert all(len(c.table) == 2 for c in ctxs)
    finally:
        v.close()


def test_the_same_device_twice_is_one_device():
    v, ctxs = _open(devices=[0, 0], n_contexts=2, pubkeys48=b"\x01" * 48)
    try:
        assert len(ctxs) == 5
        assert all(c.shared_with is ctxs[0] for c in ctxs[1:])
        assert [c.loads for c in ctxs] == [1, 0, 0, 0, 0]
    finally:
        v.close()


def test_the_option_off_loads_context_by_context():
    v, ctxs = _open(devices=[0], n_contexts=3, pubkeys48=b"\x01" * 48, share_pubkeys=False)
    try:
        assert all(c.shared_with is None for c in ctxs)
        assert [c.loads for c in ctxs] == [1, 1, 1, 1]
    finally:
        v.close()


def test_a_stand_in_without_the_method_gets_per_context_loads():
    opened = []

    class Counting(TokenCtx):
        def __init__(self, device, high_priority=False):
            super().__init__(device, high_priority, delay_s=0.0)
            self.loads = 0
            opened.append(self)

        def load_pubkeys(self, pks, width=48):
            self.loads += 1
            return super().load_pubkeys(pks, width)

    assert not hasattr(TokenCtx, "share_pubkeys")
    v = GpuBlsVerifier(devices=[0, 0], n_contexts=2, context_factory=Counting, pubkeys48=b"\x01" * 48)
    try:
        assert v._table_ctxs is None
        assert [c.loads for c in opened] == [1] * 5
    finally:
        v.close()


_JS = r"""
const {GpuBlsVerifier} = require(process.argv[1]);
function fake(withShare) {
  const log = {loads: [], shares: []};
  let next = 0;
  const addon = {
    init: (dev, high) => ({id: next++, dev, high}),
    close: () => {},
    loadPubkeys: (h, pks) => {
      log.loads.push(h.id);
      return Int32Array.from({length: pks.length / 48}, (_, i) => (pks[48 * i] === 0xff ? 1 : 0));
    },
  };
  if (withShare) addon.sharePubkeys = (h, w) => log.shares.push([h.id, w.id, h.dev === w.dev]);
  return {addon, log};
}
const out = {};
for (const [name, withShare, opts] of [["two", true, {devices: [0, 1]}], ["twice", true, {devices: [0, 0]}],
  ["off", true, {devices: [0, 0], sharePubkeys: false}], ["old", false, {devices: [0, 1]}]]) {
  const f = fake(withShare);
  const v = new GpuBlsVerifier(Object.assign({contexts: 2, addon: f.addon, uvThreadpoolSize: 64}, opts));
  v.loadPubkeys(Buffer.alloc(96, 1));
  let bad = "loaded";
  try { v.loadPubkeys(Buffer.concat([Buffer.alloc(48, 1), Buffer.alloc(48, 0xff)])); } catch (e) { bad = e.message; }
  out[name] = {loads: f.log.loads, shares: f.log.shares, tableCtxs: v.tableCtxs && v.tableCtxs.length, bad};
}
console.log(JSON.stringify(out));
"""


@pytest.mark.skipif(NODE is None, reason="node is absent")
def test_js_verifier_over_a_stand_in_addon():
    """ids: 0 the main-thread lane (device of slot 0), 1-2 slot 0's contexts, 3-4 slot 1's"""
    out = subprocess.run([NODE, "-e", _JS, str(ROOT / "integration" / "js" / "gpuBlsVerifier.js")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["two"]["shares"] == [[1, 0, True], [2, 0, True], [4, 3, True]]
    assert r["two"]["loads"] == [0, 3, 0] and r["two"]["tableCtxs"] == 2  # the bad batch stops at device 0
    assert "batch index 1" in r["two"]["bad"]
    assert r["twice"]["shares"] == [[k, 0, True] for k in (1, 2, 3, 4)]
    assert r["twice"]["loads"] == [0, 0] and r["twice"]["tableCtxs"] == 1
    for name in ("off", "old"):
        assert r[name]["shares"] == [] and r[name]["tableCtxs"] is None
        assert r[name]["loads"] == [0, 1, 2, 3, 4, 0], name  # every context, then the bad batch at the first
