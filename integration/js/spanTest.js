"use strict";
/**
 * Span sets (one field over several committees, EIP-7549) through the addon (verifySpans,
 * aggregateSpans) and GpuBlsVerifier's {type: "committee", committees: [...]} sets, on the
 * GPU.  Input: a JSON file {keys48: hex, committees: [[index...]], sets: [{committees:
 * [[group, index]...], bits: hex, list: [index...], msg, sig}], singles: [{idx, msg, sig}]}
 * (made by tests/test_napi_spans.py: each set's signature is by the keys of `list`, the
 * expansion of its bits over the concatenated committees).  Prints one JSON line of results.
 */
const fs = require("fs");
const {GpuBlsVerifier, setWeight, packRequests, packSpans} = require("./gpuBlsVerifier.js");

const hex = (h) => Buffer.from(h, "hex");
const asSpan = (s) => ({type: "committee", committees: s.committees, bits: hex(s.bits), signingRoot: hex(s.msg),
                        signature: hex(s.sig)});
const asList = (s) => ({pubkeyIndices: s.list, signingRoot: hex(s.msg), signature: hex(s.sig)});
const single = (s) => ({pubkeyIndices: [s.idx], signingRoot: hex(s.msg), signature: hex(s.sig)});
const settle = (p) => p.then((v) => v, (e) => "error: " + e.message);

async function main() {
  const data = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
  const out = {};
  // two device slots on one card, one context each, plus the main-thread lane
  const pool = new GpuBlsVerifier({devices: [0, 0], contexts: 1, warn: () => {}});
  const addon = pool.addon;
  out.addon = [typeof addon.verifySpans, typeof addon.aggregateSpans];
  pool.loadPubkeys(hex(data.keys48));
  await pool.setCommitteeGroup(0, data.committees);
  await pool.setCommitteeGroup(1, data.committees.slice().reverse());

  // every span resolves as its expanded twin does: on the pool (both slots take work),
  // batchable, and on the main-thread lane
  const ss = data.sets.map(asSpan);
  const ls = data.sets.map(asList);
  out.span = await Promise.all(ss.map((s) => settle(pool.verifySignatureSets([s], {batchable: true}))));
  out.expanded = await Promise.all(ls.map((s) => settle(pool.verifySignatureSets([s], {batchable: true}))));
  // ... and on each context by itself, whichever the routing would have picked
  out.perContext = [];
  for (const c of [pool.mainCtx].concat(pool.ctxs)) {
    const v = await addon.verifySpans(c.handle, packRequests(ss.map((s) => ({batchable: false, sets: [s]}))));
    out.perContext.push(Array.from(v));
  }
  out.mainLane = await settle(pool.verifySignatureSets(ss.slice(0, 2), {verifyOnMainThread: true}));
  // a block-like call: spans, a committee set of one committee (a one-segment span beside
  // them) and single-key sets, one job
  const one = data.sets.find((s) => s.committees.length === 1);
  const oneCommittee = {type: "committee", group: one.committees[0][0], index: one.committees[0][1], bits: hex(one.bits),
                        signingRoot: hex(one.msg), signature: hex(one.sig)};
  out.mixed = await settle(pool.verifySignatureSets(ss.slice(0, 2).concat([oneCommittee], data.singles.map(single)), {}));
  // a signature over another root; an unregistered segment; no bit anywhere; 65 segments
  out.wrong = await settle(pool.verifySignatureSets([Object.assign({}, ss[0], {signingRoot: ss[1].signingRoot})], {}));
  const unreg = ss[0].committees.slice(0, -1).concat([[3, 0]]);
  out.unregistered = await settle(pool.verifySignatureSets([Object.assign({}, ss[0], {committees: unreg})], {}));
  out.noBits = await settle(pool.verifySignatureSets([Object.assign({}, ss[0], {bits: Buffer.alloc(ss[0].bits.length)})], {}));
  const many = new Array(65).fill(ss[0].committees[0]);
  out.tooMany = await settle(pool.verifySignatureSets([Object.assign({}, ss[0], {committees: many})], {}));
  out.weights = ss.map((s) => setWeight(s, pool.groups));

  // the aggregate keys: through the verifier and through the addon on one context
  const agg = await pool.aggregateSpans(data.sets.map((s) => ({committees: s.committees, bits: hex(s.bits)})));
  out.aggKeys = agg.keys.map((k) => k.toString("hex"));
  out.aggCodes = Array.from(agg.codes);
  const raw = await addon.aggregateSpans(pool.ctxs[0].handle,
                                         packSpans([{committees: ss[0].committees, bits: Buffer.alloc(ss[0].bits.length)},
                                                    {committees: ss[0].committees, bits: ss[0].bits}]));
  out.rawCodes = Array.from(raw.codes);
  out.rawKey1 = Buffer.from(raw.keys.subarray(96, 192)).toString("hex");
  out.aggTooMany = await settle(addon.aggregateSpans(pool.ctxs[0].handle, packSpans([{committees: many, bits: Buffer.alloc(9)}])));
  await pool.close();
  console.log(JSON.stringify(out));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
