// Device tower-op self-test (bls_gpu_tower_op_test): one lane per record runs ONE function
// of the Fp6 / Fp12 tower on Fp values given as 12 little-endian 32-bit words in Montgomery
// form, exactly what production passes into these functions, and writes the function's raw
// result.  Nothing on the device converts or canonicalises around the call
// (kernels/field_ops.hpp does the same one layer down, kernels/curve_ops.hpp one layer up).
//
// Each op runs the production function in the translation-unit flavour production compiles
// it in (kernels/tower_op_ids.hpp):
//   kernels/k_selftest.hip      32-bit column product: the exact path's miller_loop and
//                               fp12_mul (pipeline.hpp pair_set, kernels/k_exact.hip)
//   kernels/k_selftest_d28.hip  BLS_FP_D28: the header functions fe_is_one calls in
//                               kernels/k_fin_simt.hip (op bit TOP_D28_FLAG)
//   kernels/k_fin_simt.hip      BLS_FP_D28: the file-local mul12m, cyc_sqr and exp_x_m,
//                               called unchanged by a kernel beside k_chunk_simt
//   kernels/k_mlq.hip           BLS_FP_D28 + BLS_FP2_PRIM: sqr12, mul_line12, fp12_mul_line2
//                               and the pair halves, by a kernel beside k_mlf
// TOP_MLQ_LINES has no kernel here: bls_gpu.hip (tower_lines_test) launches k_mlq<1> alone.
// Vectors and references: tests/_towervec.py; tests: tests/test_gpu_tower_ops.py.
#pragma once

#include "../launchers.hpp"
#include "../bls/field.hpp"
#include "tower_op_ids.hpp"

namespace bls {

static_assert(sizeof(Fp) == 48 && sizeof(Fp6) == 6 * sizeof(Fp) && sizeof(Fp12) == 12 * sizeof(Fp), "record layouts");

template <uint32_t OP>
__device__ __forceinline__ void tower_op_body(const Fp* x, Fp* y) {
  const Fp6& a6 = *reinterpret_cast<const Fp6*>(x);
  const Fp12& a12 = *reinterpret_cast<const Fp12*>(x);
  const Fp2* x2 = reinterpret_cast<const Fp2*>(x);
  if constexpr (OP == TOP_FP6_MUL) *reinterpret_cast<Fp6*>(y) = fp6_mul(a6, *reinterpret_cast<const Fp6*>(x + 6));
  else if constexpr (OP == TOP_FP6_MUL_01) *reinterpret_cast<Fp6*>(y) = fp6_mul_01(a6, x2[3], x2[4]);
  else if constexpr (OP == TOP_FP6_MUL_1) *reinterpret_cast<Fp6*>(y) = fp6_mul_1(a6, x2[3]);
  else if constexpr (OP == TOP_FP6_INV) *reinterpret_cast<Fp6*>(y) = fp6_inv(a6);
  else if constexpr (OP == TOP_FP12_MUL)
    *reinterpret_cast<Fp12*>(y) = fp12_mul(a12, *reinterpret_cast<const Fp12*>(x + 12));
  else if constexpr (OP == TOP_FP12_SQR) *reinterpret_cast<Fp12*>(y) = fp12_sqr(a12);
  else if constexpr (OP == TOP_FP12_MUL_LINE) *reinterpret_cast<Fp12*>(y) = fp12_mul_line(a12, x2[6], x2[7], x2[8]);
  else if constexpr (OP == TOP_FP12_INV) *reinterpret_cast<Fp12*>(y) = fp12_inv(a12);
  else if constexpr (OP == TOP_FP12_FROB) *reinterpret_cast<Fp12*>(y) = fp12_frob(a12);
  else if constexpr (OP == TOP_FP12_FROB2) *reinterpret_cast<Fp12*>(y) = fp12_frob2(a12);
}

template <uint32_t OP, bool D28, int IN, int OUT>
__global__ __launch_bounds__(BLS_BLOCK) void k_tower_op(const Fp* __restrict__ in, uint32_t n, Fp* __restrict__ out) {
  const uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i >= n) return;
  Fp x[IN], y[OUT];
#pragma unroll
  for (int k = 0; k < IN; ++k) x[k] = in[(size_t)IN * i + k];
  tower_op_body<OP>(x, y);
#pragma unroll
  for (int k = 0; k < OUT; ++k) out[(size_t)OUT * i + k] = y[k];
}

#if defined(BLS_FP_D28)
#define TOP_IS_D28 true
#else
#define TOP_IS_D28 false
#endif

#define TOP_CASE(OP)                                                                                  \
  case OP:                                                                                            \
    k_tower_op<OP, TOP_IS_D28, tower_op_in_fps(OP), tower_op_out_fps(OP)>                              \
        <<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(in, n, out);                                           \
    break

// launch base op `op` in this translation unit's flavour; hipErrorInvalidValue for an op
// this flavour lacks
static hipError_t tower_op_launch(uint32_t op, const Fp* in, uint32_t n, Fp* out, hipStream_t s) {
  switch (op) {
    TOP_CASE(TOP_FP6_MUL);
#if defined(BLS_FP_D28)
    TOP_CASE(TOP_FP6_INV);
    TOP_CASE(TOP_FP12_INV);
    TOP_CASE(TOP_FP12_FROB);
    TOP_CASE(TOP_FP12_FROB2);
#else
    TOP_CASE(TOP_FP6_MUL_01);
    TOP_CASE(TOP_FP6_MUL_1);
    TOP_CASE(TOP_FP12_MUL);
    TOP_CASE(TOP_FP12_SQR);
    TOP_CASE(TOP_FP12_MUL_LINE);
#endif
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bls
