"use strict";
/**
 * One key table per device through the addon (sharePubkeys, pubkeysInfo) and GpuBlsVerifier's
 * sharePubkeys option, on the GPU.  Input: a JSON file {first48: hex, later48: hex, sets:
 * [{idx, msg, sig}] over the first keys, laterSets: the same over the later keys, smMsg,
 * smSets: [{idx, sig}] signing smMsg} (made by tests/test_napi_shared_table.py).  Prints one
 * JSON line of results.
 */
const fs = require("fs");
const {GpuBlsVerifier} = require("./gpuBlsVerifier.js");

const hex = (h) => Buffer.from(h, "hex");
const wire = (s) => ({pubkeyIndices: [s.idx], signingRoot: hex(s.msg), signature: hex(s.sig)});

async function main() {
  const data = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
  const out = {};
  const pool = new GpuBlsVerifier({contexts: 3, warn: () => {}});
  const addon = pool.addon;
  out.addon = [typeof addon.sharePubkeys, typeof addon.pubkeysInfo];
  const all = [pool.mainCtx].concat(pool.ctxs);
  const infos = () => all.map((c) => addon.pubkeysInfo(c.handle));
  out.tableCtxs = pool.tableCtxs.length;

  // one load for the four contexts
  let loads = 0;
  // (the addon's own properties are neither enumerable nor writable: a derived object)
  pool.addon = Object.create(addon, {loadPubkeys: {value: (...a) => (loads++, addon.loadPubkeys(...a))}});
  pool.loadPubkeys(hex(data.first48));
  out.loadsFirst = loads;
  out.first = infos();

  const sets = data.sets.map(wire);
  out.batchable = await Promise.all(sets.map((s) => pool.verifySignatureSets([s], {batchable: true})));
  out.mainLane = await pool.verifySignatureSets(sets.slice(0, 3), {verifyOnMainThread: true});
  const wrong = Object.assign({}, sets[0], {signingRoot: sets[1].signingRoot});
  out.wrong = await pool.verifySignatureSets([wrong, sets[2]], {batchable: true});
  out.sameMessage = await pool.verifySignatureSetsSameMessage(
    data.smSets.map((s) => ({publicKey: s.idx, signature: hex(s.sig)})), hex(data.smMsg));

  // a later load appends once, and every context verifies the new keys
  loads = 0;
  pool.loadPubkeys(hex(data.later48));
  out.loadsLater = loads;
  out.later = infos();
  const laterSets = data.laterSets.map(wire);
  out.laterPool = await Promise.all(laterSets.map((s) => pool.verifySignatureSets([s], {batchable: true})));
  out.laterMain = await pool.verifySignatureSets(laterSets, {verifyOnMainThread: true});

  // a batch with an undecodable key appends nothing, for every sharer
  const bad = Buffer.concat([hex(data.later48).slice(0, 48), Buffer.alloc(48, 0xff)]);
  out.badLoad = (() => {
    try {
      pool.loadPubkeys(bad);
      return "loaded";
    } catch (e) {
      return e.message;
    }
  })();
  out.afterBad = infos().map((i) => i.nKeys);

  // refusals: into a context that holds keys, with itself
  const refuse = (a, b) => {
    try {
      addon.sharePubkeys(a, b);
      return "shared";
    } catch (e) {
      return e.message;
    }
  };
  const lone = addon.init(0, false);
  addon.loadPubkeys(lone, hex(data.first48).slice(0, 48), 48);
  out.refuseHoldsKeys = refuse(lone, pool.mainCtx.handle);
  out.refuseSelf = refuse(lone, lone);
  out.again = refuse(pool.ctxs[0].handle, pool.mainCtx.handle); // already peers: fine
  out.loneInfo = addon.pubkeysInfo(lone);
  addon.close(lone);
  await pool.close();

  // the option off: a table per context, a load per context
  const own = new GpuBlsVerifier({contexts: 3, sharePubkeys: false, warn: () => {}});
  own.loadPubkeys(hex(data.first48));
  out.ownIds = [own.mainCtx].concat(own.ctxs).map((c) => addon.pubkeysInfo(c.handle).tableId);
  out.ownTableCtxs = own.tableCtxs;
  out.ownVerdict = await own.verifySignatureSets(sets.slice(0, 2), {batchable: true});
  await own.close();
  console.log(JSON.stringify(out));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
