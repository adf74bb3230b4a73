"use strict";
/**
 * GpuBlsVerifier.verifyDeposits and the addon's verifyDeposits on the GPU
 * (processDeposit.ts:48-65).  Input: a JSON file {forkVersion: hex, domain: hex, kat1:
 * deposit, deposits: [deposit..]} with deposit = {pubkey, wc, amount (decimal string),
 * signature} in hex (made by tests/test_napi_deposits.py, which also holds the verdicts
 * Python computed).  Prints one JSON line of results.
 */
const fs = require("fs");
const {GpuBlsVerifier, packDeposits, depositDomain} = require("./gpuBlsVerifier.js");

function deposit(d) {
  return {pubkey: Buffer.from(d.pubkey, "hex"), withdrawalCredentials: Buffer.from(d.wc, "hex"),
          amount: BigInt(d.amount), signature: Buffer.from(d.signature, "hex")};
}

async function main() {
  const data = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
  const forkVersion = Buffer.from(data.forkVersion, "hex");
  const kat1 = deposit(data.kat1);
  const deposits = data.deposits.map(deposit);
  const pool = new GpuBlsVerifier({contexts: 1});
  const out = {addon: typeof pool.addon.verifyDeposits};
  out.domain = depositDomain(forkVersion).toString("hex");

  // KAT-1, and the same deposit with its amount off by one: resolves false, no rejection
  out.kat1 = await pool.verifyDeposits([kat1], {forkVersion});
  out.kat1Tampered = await pool.verifyDeposits([Object.assign({}, kat1, {amount: kat1.amount + 1n})], {forkVersion})
    .then((v) => v, (e) => "rejected: " + e.message);

  // the mixed list, by fork version and by domain; every invalid deposit resolves false
  out.mixed = await pool.verifyDeposits(deposits, {forkVersion}).then((v) => v, (e) => "rejected: " + e.message);
  out.mixedByDomain = await pool.verifyDeposits(deposits, {domain: Buffer.from(data.domain, "hex")});
  out.empty = await pool.verifyDeposits([], {forkVersion});

  // the addon call itself: the codes per deposit and the worker bookkeeping
  const req = packDeposits(deposits, Buffer.from(data.domain, "hex"));
  const v = await pool.addon.verifyDeposits(pool.ctxs[0].handle, req);
  out.native = {verdicts: Array.from(v), nChunks: v.nChunks, batchRetries: v.batchRetries};

  // a signature of the wrong length is an invalid deposit, not an exception
  const short = Object.assign({}, deposits[1], {signature: deposits[1].signature.subarray(0, 95)});
  out.shortSignature = await pool.verifyDeposits([deposits[1], short], {forkVersion});
  // neither a fork version nor a domain: the caller's error rejects
  out.noDomain = await pool.verifyDeposits(deposits, {}).then(() => "resolved", (e) => e.message);

  await pool.close();
  console.log(JSON.stringify(out));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
