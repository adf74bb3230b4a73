// Op ids and record shapes of the device tower-op self-test (kernels/tower_ops.hpp), apart
// from its kernels so that kernels/k_mlq.hip and kernels/k_fin_simt.hip can take them
// without the field self-test.
#pragma once

#include <stdint.h>

namespace bls {

// op ids of bls_gpu_tower_op_test (include/lodestar_bls.h; TOP_D28_FLAG selects the flavour).
// Records are whole Fp values (12 words each, Montgomery form); an Fp6 is 6 Fp, an Fp12 12 Fp
// in memory order (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2), a line l0, l2, l3 (6 Fp).
// The flavours are the ones a production kernel compiles the function in:
//   cols  pair_set's miller_loop and fp12_mul on the exact path (kernels/k_exact.hip)
//   d28   fe_is_one's callees in kernels/k_fin_simt.hip
enum : uint32_t {
  // bls/field.hpp, by kernels/tower_ops.hpp
  TOP_FP6_MUL = 0,        // fp6_mul: a, b -> Fp6                                   (cols, d28)
  TOP_FP6_MUL_01,         // fp6_mul_01: a, d0, d1 -> Fp6                           (cols)
  TOP_FP6_MUL_1,          // fp6_mul_1: a, d1 -> Fp6                                (cols)
  TOP_FP6_INV,            // fp6_inv: a -> Fp6                                      (d28)
  TOP_FP12_MUL,           // fp12_mul: a, b -> Fp12                                 (cols)
  TOP_FP12_SQR,           // fp12_sqr: a -> Fp12                                    (cols)
  TOP_FP12_MUL_LINE,      // fp12_mul_line: f, line -> Fp12                         (cols)
  TOP_FP12_INV,           // fp12_inv: a -> Fp12                                    (d28)
  TOP_FP12_FROB,          // fp12_frob: a -> Fp12                                   (d28)
  TOP_FP12_FROB2,         // fp12_frob2: a -> Fp12                                  (d28)
  // kernels/k_fin_simt.hip's file-local functions, by k_tower_op_fin beside k_chunk_simt (d28)
  TOP_FIN_MUL12M,         // mul12m<false>: a, m (m read from memory) -> Fp12
  TOP_FIN_MUL12M_CONJ,    // mul12m<true>: a, m -> a conj(m)
  TOP_FIN_CYC_SQR,        // cyc_sqr: f (cyclotomic) -> Fp12
  TOP_FIN_EXP_X_M,        // exp_x_m: base (cyclotomic, in memory) -> base^x in memory
  // kernels/k_mlq.hip's, by k_tower_op_mlq beside k_mlf (d28 + the Fp2 primitive)
  TOP_MLQ_SQR12,          // sqr12: a -> Fp12
  TOP_MLQ_MUL_LINE12,     // mul_line12: f, line -> Fp12
  TOP_MLQ_MUL_LINE2,      // fp12_mul_line2: f, line, line -> Fp12
  TOP_MLQ_SQR12_PAIR,     // sqr12_pair on lanes 2k, 2k + 1: a -> both lanes' Fp12
  TOP_MLQ_MUL_LINE12_PAIR,  // mul_line12_pair likewise: f, line -> both lanes' Fp12
  // no kernel of its own: bls_gpu.hip (tower_lines_test) fills a zeroed PipeBufs and launches
  // k_mlq<1> alone
  TOP_MLQ_LINES,          // RP (Jacobian G1: x, y, z), HQ (4 Fp) -> the item's 68 lines
  TOP_COUNT
};
#define TOP_LINES_MAX 64u     // items per TOP_MLQ_LINES call
#define TOP_LINE_EVENTS 68    // 63 doublings + 5 additions (kernels/k_mlq.hip ML_EVENTS)
#define TOP_D28_FLAG 0x100u

// record sizes in Fp values (12 words each)
constexpr int tower_op_in_fps(uint32_t op) {
  return op == TOP_FP6_MUL ? 12 : op == TOP_FP6_MUL_01 ? 10 : op == TOP_FP6_MUL_1 ? 8 : op == TOP_FP6_INV ? 6
         : op == TOP_FP12_MUL || op == TOP_FIN_MUL12M || op == TOP_FIN_MUL12M_CONJ || op == TOP_MLQ_MUL_LINE2 ? 24
         : op == TOP_FP12_MUL_LINE || op == TOP_MLQ_MUL_LINE12 || op == TOP_MLQ_MUL_LINE12_PAIR ? 18
         : op == TOP_MLQ_LINES ? 7 : 12;
}
constexpr int tower_op_out_fps(uint32_t op) {
  return op <= TOP_FP6_INV ? 6 : op == TOP_MLQ_SQR12_PAIR || op == TOP_MLQ_MUL_LINE12_PAIR ? 24
         : op == TOP_MLQ_LINES ? 6 * TOP_LINE_EVENTS : 12;
}
// the flavours an op exists in: bit 0 the 32-bit column product, bit 1 the 28-bit-digit one
constexpr uint32_t tower_op_flavours(uint32_t op) {
  return op == TOP_FP6_MUL ? 3u
         : op == TOP_FP6_MUL_01 || op == TOP_FP6_MUL_1 || op == TOP_FP12_MUL || op == TOP_FP12_SQR ||
                 op == TOP_FP12_MUL_LINE
             ? 1u
             : 2u;
}
// the ops of kernels/k_fin_simt.hip (launch_k_tower_op_fin) and of kernels/k_mlq.hip
// (launch_k_tower_op_mlq)
constexpr bool tower_op_in_fin_tu(uint32_t op) { return op >= TOP_FIN_MUL12M && op <= TOP_FIN_EXP_X_M; }
constexpr bool tower_op_in_mlq_tu(uint32_t op) { return op >= TOP_MLQ_SQR12 && op <= TOP_MLQ_MUL_LINE12_PAIR; }
constexpr bool tower_op_is_pair(uint32_t op) { return op == TOP_MLQ_SQR12_PAIR || op == TOP_MLQ_MUL_LINE12_PAIR; }
// the op bls_gpu.hip runs through k_mlq itself
constexpr bool tower_op_on_host(uint32_t op) { return op == TOP_MLQ_LINES; }

}  // namespace bls
