"use strict";
/**
 * Committee-bitfield sets through the addon (setCommitteeGroup, committeeGroupInfo,
 * verifyCommittees) and GpuBlsVerifier.setCommitteeGroup / {type: "committee"} sets, on the
 * GPU.  Input: a JSON file {keys48: hex, committees: [[index...]], later: [[index...]],
 * sets: [{group, index, bits: hex, list: [index...], msg, sig}], singles: [{idx, msg, sig}]}
 * (made by tests/test_napi_committees.py: each set's signature is by the keys of `list`, the
 * expansion of its bits).  Prints one JSON line of results.
 */
const fs = require("fs");
const {GpuBlsVerifier, setWeight, packRequests} = require("./gpuBlsVerifier.js");

const hex = (h) => Buffer.from(h, "hex");
const asCommittee = (s) => ({type: "committee", group: s.group, index: s.index, bits: hex(s.bits),
                             signingRoot: hex(s.msg), signature: hex(s.sig)});
const asList = (s) => ({pubkeyIndices: s.list, signingRoot: hex(s.msg), signature: hex(s.sig)});
const single = (s) => ({pubkeyIndices: [s.idx], signingRoot: hex(s.msg), signature: hex(s.sig)});
const settle = (p) => p.then((v) => v, (e) => "error: " + e.message);

async function main() {
  const data = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
  const out = {};
  // two device slots on one card, one context each, plus the main-thread lane
  const pool = new GpuBlsVerifier({devices: [0, 0], contexts: 1, warn: () => {}});
  const addon = pool.addon;
  out.addon = [typeof addon.setCommitteeGroup, typeof addon.committeeGroupInfo, typeof addon.verifyCommittees];
  pool.loadPubkeys(hex(data.keys48));
  const infos = (g) => [pool.mainCtx].concat(pool.ctxs).map((c) => addon.committeeGroupInfo(c.handle, g));

  out.before = infos(0);
  await pool.setCommitteeGroup(0, data.committees);
  out.after = infos(0);

  // every committee set resolves as its expanded twin does: on the pool (both slots take
  // work), batchable, and on the main-thread lane
  const cs = data.sets.map(asCommittee);
  const ls = data.sets.map(asList);
  out.committee = await Promise.all(cs.map((s) => settle(pool.verifySignatureSets([s], {batchable: true}))));
  out.expanded = await Promise.all(ls.map((s) => settle(pool.verifySignatureSets([s], {batchable: true}))));
  // ... and on each context by itself, whichever the routing would have picked
  out.perContext = [];
  for (const c of [pool.mainCtx].concat(pool.ctxs)) {
    const v = await addon.verifyCommittees(c.handle, packRequests(cs.map((s) => ({batchable: false, sets: [s]}))));
    out.perContext.push(Array.from(v));
  }
  out.mainLane = await settle(pool.verifySignatureSets(cs.slice(0, 2), {verifyOnMainThread: true}));
  // a block-like call: committee sets beside single-key sets, one job
  out.mixed = await settle(pool.verifySignatureSets(cs.slice(0, 2).concat(data.singles.map(single)), {}));
  // a signature over another root; an unregistered group; no bits set
  const wrong = Object.assign({}, cs[0], {signingRoot: cs[1].signingRoot});
  out.wrong = await settle(pool.verifySignatureSets([wrong], {}));
  out.unregistered = await settle(pool.verifySignatureSets([Object.assign({}, cs[0], {group: 3})], {}));
  out.noBits = await settle(pool.verifySignatureSets([Object.assign({}, cs[0], {bits: Buffer.alloc(cs[0].bits.length)})], {}));
  out.weights = cs.map((s) => setWeight(s, pool.groups));

  // a rejected registration (a member past the table) changes no context
  out.rejected = await settle(pool.setCommitteeGroup(0, [[0, 1, 1 << 20]]));
  out.afterRejected = infos(0);
  out.stillVerifies = await settle(pool.verifySignatureSets([cs[0]], {}));

  // a context opened after the registration has the group
  const c = await pool.addContext(1);
  out.laterInfo = addon.committeeGroupInfo(c.handle, 0);
  const v = await addon.verifyCommittees(c.handle, packRequests([{batchable: false, sets: [cs[1]]}]));
  out.laterVerdict = Array.from(v);

  // replaced: the same reference now names other members
  await pool.setCommitteeGroup(0, data.later);
  out.replacedInfo = infos(0);
  out.oldSetAfterReplace = await settle(pool.verifySignatureSets([cs[0]], {}));
  await pool.setCommitteeGroup(0, []);
  out.dropped = infos(0);
  await pool.close();
  console.log(JSON.stringify(out));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
