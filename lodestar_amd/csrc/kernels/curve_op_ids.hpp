// Op ids and record shapes of the device curve-op self-test (kernels/curve_ops.hpp), apart
// from its kernels so that kernels/k_chain.hip can take them without the field self-test.
#pragma once

#include <stdint.h>

namespace bls {

// op ids of bls_gpu_curve_op_test (include/lodestar_bls.h; COP_D28_FLAG selects the flavour)
enum : uint32_t {
  COP_FROM_BE64 = 0,   // fp_from_be64_words: 16 big-endian words -> Fp            (cols, d28)
  COP_H2F,             // hash_to_field_fp2_x2: 8 message words -> u0, u1          (cols, d28)
  COP_SSWU,            // map_to_curve_sswu: u -> x, y                             (cols)
  COP_SSWU_FAST,       // map_to_curve_sswu_fast: u -> ok word, x, y               (d28)
  COP_ISO_AFF,         // iso_map_g2: x, y -> inf word, x, y                       (cols)
  COP_ISO_JAC,         // k_chain.hip iso_jac_nl: x, y -> X, Y, Z                  (d28 + prim)
  COP_CLEAR_COFACTOR,  // g2_clear_cofactor + jac_to_aff: inf, x, y -> inf, x, y   (cols)
  COP_CHAIN_H,         // k_chain.hip chain_role_h: q0, q1 -> chain_st byte, HQ    (d28 + prim)
  // the two below run the production launchers over a PipeBufs that bls_gpu.hip fills with
  // the records alone (curve_miller_test / curve_fe_test): no kernel of their own
  COP_MILLER,          // launch_k_mlqf: RP (Jacobian G1), HQ, domain, per_lane -> f (12 Fp) (d28 + prim)
  COP_FE,              // launch_k_chunk_simt, launch_k_chunk_coop: F (12 Fp) -> both chunk_ok  (d28)
  COP_COUNT
};
#define COP_MILLER_MAX 1024u  // items per call (the line buffer is 19,584 B per item)
#define COP_D28_FLAG 0x100u

constexpr int curve_op_in_words(uint32_t op) {
  return op == COP_FROM_BE64 ? 16 : op == COP_H2F ? 8 : op == COP_SSWU || op == COP_SSWU_FAST ? 24
         : op == COP_CLEAR_COFACTOR ? 49 : op == COP_CHAIN_H ? 96 : op == COP_MILLER ? 86 : op == COP_FE ? 144 : 48;
}
constexpr int curve_op_out_words(uint32_t op) {
  return op == COP_FROM_BE64 ? 12 : op == COP_H2F || op == COP_SSWU ? 48 : op == COP_ISO_JAC ? 72
         : op == COP_MILLER ? 144 : op == COP_FE ? 2 : 49;
}
// the flavours an op exists in: bit 0 the 32-bit column product, bit 1 the 28-bit-digit one
constexpr uint32_t curve_op_flavours(uint32_t op) {
  return op == COP_FROM_BE64 || op == COP_H2F ? 3u
         : op == COP_SSWU || op == COP_ISO_AFF || op == COP_CLEAR_COFACTOR ? 1u : 2u;
}
// the ops of kernels/k_chain.hip (launch_k_curve_op_chain)
constexpr bool curve_op_in_chain_tu(uint32_t op) { return op == COP_ISO_JAC || op == COP_CHAIN_H; }
// the ops bls_gpu.hip runs through the production launchers
constexpr bool curve_op_on_host(uint32_t op) { return op == COP_MILLER || op == COP_FE; }

}  // namespace bls
