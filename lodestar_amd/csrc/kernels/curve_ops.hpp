// Device curve-op self-test (bls_gpu_curve_op_test): one lane per record runs ONE curve-
// level function of the verify path -- hash_to_field, the two SSWU maps, the isogeny in
// both forms, the cofactor clearing, k_chain's whole role 0 -- on Fp values given as 12
// little-endian 32-bit words in Montgomery form, exactly what production passes between
// these kernels, and writes the function's raw result.  Nothing on the device converts or
// canonicalises around the call (kernels/field_ops.hpp does the same one layer down).
//
// Each op runs the production function in the translation-unit flavour production compiles
// it in:
//   kernels/k_selftest.hip      32-bit column product, as k_h2c, k_sign and the exact path
//   kernels/k_selftest_d28.hip  BLS_FP_D28, as k_pre (op bit COP_D28_FLAG)
//   kernels/k_chain.hip         BLS_FP_D28 + BLS_FP2_PRIM: the file-local iso_jac_nl and
//                               chain_role_h, called unchanged by a kernel beside k_chain
// COP_MILLER and COP_FE have no kernel here: bls_gpu.hip (curve_miller_test, curve_fe_test)
// fills a zeroed PipeBufs with the records and calls launch_k_mlqf, launch_k_chunk_simt and
// launch_k_chunk_coop.
// Vectors and references: tests/_curvevec.py; tests: tests/test_gpu_curve_ops.py.
#pragma once

#include "../launchers.hpp"
#include "../bls/hash_to_curve.hpp"
#include "curve_op_ids.hpp"
#include "field_ops.hpp"

namespace bls {

template <uint32_t OP>
__device__ __forceinline__ void curve_op_body(const uint32_t* x, uint32_t* y) {
  if constexpr (OP == COP_FROM_BE64) fop_st(y, 0, fp_from_be64_words(x));
  else if constexpr (OP == COP_H2F) {
    Fp2 u0, u1;
    hash_to_field_fp2_x2(x, u0, u1);
    fop_st2(y, 0, u0);
    fop_st2(y, 1, u1);
  } else if constexpr (OP == COP_SSWU) {
    const G2A r = map_to_curve_sswu(fop_ld2(x, 0));
    fop_st2(y, 0, r.x);
    fop_st2(y, 1, r.y);
  } else if constexpr (OP == COP_SSWU_FAST) {
    Fp2 px = fp2_zero(), py = fp2_zero();
    y[0] = map_to_curve_sswu_fast(fop_ld2(x, 0), px, py) ? 1u : 0u;
    fop_st2(y + 1, 0, px);
    fop_st2(y + 1, 1, py);
  } else if constexpr (OP == COP_ISO_AFF || OP == COP_CLEAR_COFACTOR) {
    G2A p;
    if constexpr (OP == COP_ISO_AFF) {
      p.inf = false;
      p.x = fop_ld2(x, 0);
      p.y = fop_ld2(x, 1);
    } else {
      p.inf = x[0] != 0;
      p.x = fop_ld2(x + 1, 0);
      p.y = fop_ld2(x + 1, 1);
    }
    G2A r;
    if constexpr (OP == COP_ISO_AFF) r = iso_map_g2(p);
    else r = jac_to_aff(g2_clear_cofactor(jac_from_aff(p)));
    y[0] = r.inf ? 1u : 0u;
    fop_st2(y + 1, 0, r.x);
    fop_st2(y + 1, 1, r.y);
  }
}

template <uint32_t OP, bool D28, int IN, int OUT>
__global__ __launch_bounds__(BLS_BLOCK) void k_curve_op(const uint32_t* __restrict__ in, uint32_t n,
                                                        uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t x[IN], y[OUT];
#pragma unroll
  for (int k = 0; k < IN; ++k) x[k] = in[(size_t)IN * i + k];
#pragma unroll
  for (int k = 0; k < OUT; ++k) y[k] = 0;
  curve_op_body<OP>(x, y);
#pragma unroll
  for (int k = 0; k < OUT; ++k) out[(size_t)OUT * i + k] = y[k];
}

#define COP_CASE(OP)                                                                                    \
  case OP:                                                                                              \
    k_curve_op<OP, FOP_IS_D28, curve_op_in_words(OP), curve_op_out_words(OP)>                            \
        <<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(in, n, out);                                             \
    break

// launch base op `op` in this translation unit's flavour; hipErrorInvalidValue for an op
// this flavour lacks
static hipError_t curve_op_launch(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s) {
  switch (op) {
    COP_CASE(COP_FROM_BE64);
    COP_CASE(COP_H2F);
#if defined(BLS_FP_D28)
    COP_CASE(COP_SSWU_FAST);
#else
    COP_CASE(COP_SSWU);
    COP_CASE(COP_ISO_AFF);
    COP_CASE(COP_CLEAR_COFACTOR);
#endif
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bls
