// Per-deposit stage bodies of bls_gpu_verify_deposits (include/lodestar_bls.h), shared by
// the front kernel (kernels/k_deposit.hip) and the CPU test program
// (tests/native/deposit_host.cpp).
//
// processDeposit (state-transition/src/block/processDeposit.ts:48-65) checks a deposit
// of an unknown validator inside one try block: PublicKey.fromBytes(pubkey, validate),
// Signature.fromBytes(signature, validate), verify(computeSigningRoot(DepositMessage,
// domain)).  The two bodies here are its first step and its message; the signature and
// the pairing are the verify pass's own stages (bls/pipeline.hpp).
#pragma once

#include "pipeline.hpp"
#include "ssz_tree.hpp"

namespace bls {

// what the front kernel reads beside PipeBufs: the call's four input arrays, as staged
struct DepositBufs {
  const uint8_t* pubkeys48;  // n * 48 compressed G1, untrusted
  const uint8_t* wc;         // n * 32 withdrawal credentials
  const uint8_t* amounts;    // n * 8 little-endian Gwei
  const uint8_t* domain;     // 32
  uint8_t* roots;            // n * 32: the pass's message buffer (PipeBufs::msgs), written here
};

// computeSigningRoot(DepositMessage{pubkey, wc, amount}, domain) (signingRoot.ts:7-13):
// 5 hash_pair = 10 SHA-256 compressions
BLS_HD void stage_deposit_root(const uint8_t* pubkey48, const uint8_t* wc32, const uint8_t* amount8,
                               const uint8_t* domain32, uint8_t* out32) {
  const Chunk r = hash_pair(deposit_message_root(pubkey48, wc32, amount8), load_chunk(domain32, 32));
  store_chunk(r, out32);
}

// KeyValidate of an untrusted compressed key (blst PublicKey.fromBytes(bytes, validate =
// true) [ext]): decode (BAD_ENCODING / POINT_NOT_ON_CURVE), PK_IS_INFINITY, then Scott's
// subgroup test (POINT_NOT_IN_GROUP).  `out` is the decoded point whenever the bytes
// decode -- also for a point outside G1, so the code says whether it may be used.
BLS_HD int32_t stage_deposit_key(const uint8_t* pubkey48, G1A& out) {
  int32_t c = g1_decompress48(pubkey48, out);
  if (c != BLS_OK) {
    out.inf = true;
    out.x = fp_zero();
    out.y = fp_zero();
    return c;
  }
  if (out.inf) return BLS_PK_IS_INFINITY;
  return g1_in_subgroup(out) ? BLS_OK : BLS_POINT_NOT_IN_GROUP;
}

// The key stage of a deposit call: what stage_pk leaves for the later stages.  On any code
// the point handed on is the point at infinity, so a key outside G1 never reaches a
// random-scalar product (the later stages skip a set whose pk_status is not OK as well).
BLS_HD void stage_deposit_pk(const PipeBufs& b, const DepositBufs& d, uint32_t i) {
  if (i >= b.n_sets) return;
  G1A a;
  const int32_t c = stage_deposit_key(d.pubkeys48 + 48ull * i, a);
  b.pk[i] = c == BLS_OK ? jac_from_aff(a) : jac_infinity<Fp>();
  b.pk_status[i] = c;
  if (b.pk_inf) b.pk_inf[i] = 0;  // (an infinity key is an error code here, not a flag)
}

}  // namespace bls
