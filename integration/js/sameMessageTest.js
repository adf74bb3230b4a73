"use strict";
/**
 * IBlsVerifier.verifySignatureSetsSameMessage through GpuBlsVerifier and the addon's
 * verifySameMessage on the GPU.  Input: a JSON file {pubkeys48: hex, jobs: [{msg, idx:
 * [..], sigs: [hex..]}, {..}], raw96: hex of jobs[1]'s first key, uncompressed} (made by
 * tests/test_gpu_same_message.py).  Prints one JSON line of results.
 */
const fs = require("fs");
const {GpuBlsVerifier, packSameMessage} = require("./gpuBlsVerifier.js");

async function main() {
  const data = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
  const jobs = data.jobs.map((j) => ({
    message: Buffer.from(j.msg, "hex"),
    sets: j.idx.map((ix, k) => ({publicKey: ix, signature: Buffer.from(j.sigs[k], "hex")})),
  }));
  const pool = new GpuBlsVerifier({contexts: 1});
  pool.loadPubkeys(Buffer.from(data.pubkeys48, "hex"));
  const out = {addon: typeof pool.addon.verifySameMessage};

  // one call; then two calls queued together, which one context takes in one native call
  out.single = await pool.verifySignatureSetsSameMessage(jobs[0].sets, jobs[0].message, {});
  const before = pool.stats.jobGroupsStarted;
  out.together = await Promise.all(jobs.map((j) => pool.verifySignatureSetsSameMessage(j.sets, j.message)));
  out.togetherCalls = pool.stats.jobGroupsStarted - before;

  // the addon call itself: verdict codes per set and the worker bookkeeping
  const req = packSameMessage(jobs.map((j) => ({
    message: j.message, indices: j.sets.map((s) => s.publicKey), signatures: j.sets.map((s) => s.signature)})));
  const v = await pool.addon.verifySameMessage(pool.ctxs[0].handle, req);
  out.native = {verdicts: Array.from(v), stats: {nChunks: v.nChunks, batchRetries: v.batchRetries,
    batchSigsSuccess: v.batchSigsSuccess, nIndividual: v.nIndividual}};

  // a raw key and an index list go through the existing path as one-set requests; the
  // third set carries another set's signature
  const b = jobs[1];
  out.mixed = await pool.verifySignatureSetsSameMessage([
    {publicKey: Buffer.from(data.raw96, "hex"), signature: b.sets[0].signature},
    {publicKey: b.sets[1].publicKey, signature: b.sets[1].signature},
    {publicKey: [b.sets[2].publicKey], signature: b.sets[3].signature},
  ], b.message);
  out.empty = await pool.verifySignatureSetsSameMessage([], b.message);

  // an empty job is refused by the library (-2), the promise rejects with its message
  const bad = packSameMessage([{message: b.message, indices: [], signatures: []}]);
  out.emptyJob = await pool.addon.verifySameMessage(pool.ctxs[0].handle, bad).then(() => "resolved", (e) => e.message);

  await pool.close();
  console.log(JSON.stringify(out));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
