// Device field-op self-test (bls_gpu_field_op_test): one lane per record runs ONE field
// primitive on raw little-endian 32-bit words and writes its raw result -- no
// fp_to_mont / fp_from_mont / fp_from_be48 around it, so non-canonical operands reach
// the function under test untouched and a broken product cannot hide in a conversion.
//
// Included by kernels/k_selftest.hip (the 32-bit column product) and by
// kernels/k_selftest_d28.hip (BLS_FP_D28: the 28-bit-digit product of the verify path);
// the kernels carry the flavour in their template arguments, so the two translation
// units' instantiations are different symbols.  Vectors and references:
// tests/_fieldvec.py; tests: tests/test_gpu_field_ops.py.
#pragma once

#include "../launchers.hpp"
#include "../bls/selftest_ops.hpp"

static_assert(BLS_BLOCK == 64, "one wavefront per block (the Fp2 primitive's LDS slot, FOP_FP2_*_W)");

namespace bls {

// op ids of bls_gpu_field_op_test (include/lodestar_bls.h; BLS_FIELD_OP_D28 selects the TU)
enum : uint32_t {
  FOP_ADD = 0,
  FOP_SUB,
  FOP_NEG,
  FOP_DBL,
  FOP_HALF,
  FOP_ADD_NR,
  FOP_SUB_NR,
  FOP_REDUCE_ONCE,
  FOP_REDUCE_2P,
  FOP_CANON3,
  FOP_MUL,
  FOP_SQR,
  FOP_MUL_LAZY,
  FOP_SQR_D28_LAZY,
  FOP_FP2_MUL_D28,
  FOP_FP2_SQR_D28,
  FOP_FP2_MUL,
  FOP_FP2_SQR,
  FOP_FP2_MUL_S,
  FOP_LZ_MUL_RAW,
  FOP_LZ_SQR_RAW,
  FOP_LZ_FP_OPS,
  FOP_LZ_FP2_OPS,
  FOP_INV,
  FOP_INV_GCD,
  FOP_SQRT,
  FOP_FP2_INV,
  FOP_FP2_SQRT,
  FOP_LIN8,
  FOP_FP2_MUL_W,    // fp2_mul_prim: the out-of-line lazy Fp2 product, LDS slot included
  FOP_FP2_SQR_W,    // fp2_sqr_prim
  FOP_FP2_CHAIN_W,  // four dependent products through the same slot
  FOP_PREDS,        // sf_preds: the comparison predicates on one raw pair, one bit each (both TUs)
  FOP_COUNT
};
#define FOP_D28_FLAG 0x100u
#define FOP_LIN8_IN 102  // 8 x 12 value words, 4 words of 8 int16 coefficients, n, single

// record sizes in 32-bit words, by base op id
constexpr int field_op_in_words(uint32_t op) {
  return op == FOP_NEG || op == FOP_DBL || op == FOP_HALF || op == FOP_REDUCE_ONCE || op == FOP_REDUCE_2P ||
                 op == FOP_CANON3 || op == FOP_SQR || op == FOP_SQR_D28_LAZY || op == FOP_INV ||
                 op == FOP_INV_GCD || op == FOP_SQRT
             ? 12
         : op == FOP_FP2_MUL_D28 || op == FOP_FP2_MUL || op == FOP_FP2_MUL_S || op == FOP_LZ_FP2_OPS ||
                 op == FOP_FP2_MUL_W || op == FOP_FP2_CHAIN_W
             ? 48
         : op == FOP_LZ_MUL_RAW                                                                        ? 28
         : op == FOP_LZ_SQR_RAW                                                                        ? 14
         : op == FOP_LIN8                                                                              ? FOP_LIN8_IN
                                                                                                       : 24;
}
constexpr int field_op_out_words(uint32_t op) {
  return op == FOP_FP2_MUL_D28 || op == FOP_FP2_SQR_D28 || op == FOP_FP2_MUL || op == FOP_FP2_SQR ||
                 op == FOP_FP2_MUL_S || op == FOP_FP2_INV || op == FOP_FP2_MUL_W || op == FOP_FP2_SQR_W ||
                 op == FOP_FP2_CHAIN_W
             ? 24
         : op == FOP_LZ_MUL_RAW || op == FOP_LZ_SQR_RAW ? 14
         : op == FOP_LZ_FP_OPS                          ? 120
         : op == FOP_LZ_FP2_OPS                         ? 144
         : op == FOP_SQRT                               ? 13
         : op == FOP_FP2_SQRT                           ? 25
         : op == FOP_PREDS                              ? 1
                                                        : 12;
}

// ops only the 28-bit-digit translation unit has
constexpr bool field_op_d28_only(uint32_t op) {
  return op == FOP_CANON3 || (op >= FOP_SQR_D28_LAZY && op != FOP_PREDS);
}

#if defined(BLS_FP_D28)
#define FOP_IS_D28 true
#else
#define FOP_IS_D28 false
#endif

__device__ __forceinline__ Fp fop_ld(const uint32_t* w, int k) {
  Fp r;
#pragma unroll
  for (int i = 0; i < 12; ++i) r.l[i] = w[12 * k + i];
  return r;
}
__device__ __forceinline__ void fop_st(uint32_t* w, int k, const Fp& v) {
#pragma unroll
  for (int i = 0; i < 12; ++i) w[12 * k + i] = v.l[i];
}
__device__ __forceinline__ Fp2 fop_ld2(const uint32_t* w, int k) { return Fp2{fop_ld(w, 2 * k), fop_ld(w, 2 * k + 1)}; }
__device__ __forceinline__ void fop_st2(uint32_t* w, int k, const Fp2& v) {
  fop_st(w, 2 * k, v.c0);
  fop_st(w, 2 * k + 1, v.c1);
}

template <uint32_t OP, bool D28>
__device__ __forceinline__ void field_op_body(const uint32_t* x, uint32_t* y) {
  if constexpr (OP == FOP_ADD) fop_st(y, 0, fp_add(fop_ld(x, 0), fop_ld(x, 1)));
  else if constexpr (OP == FOP_SUB) fop_st(y, 0, fp_sub(fop_ld(x, 0), fop_ld(x, 1)));
  else if constexpr (OP == FOP_NEG) fop_st(y, 0, fp_neg(fop_ld(x, 0)));
  else if constexpr (OP == FOP_DBL) fop_st(y, 0, fp_dbl(fop_ld(x, 0)));
  else if constexpr (OP == FOP_HALF) fop_st(y, 0, fp_half(fop_ld(x, 0)));
  else if constexpr (OP == FOP_ADD_NR) fop_st(y, 0, fp_add_nr(fop_ld(x, 0), fop_ld(x, 1)));
  else if constexpr (OP == FOP_SUB_NR) fop_st(y, 0, fp_sub_nr(fop_ld(x, 0), fop_ld(x, 1)));
  else if constexpr (OP == FOP_REDUCE_ONCE) fop_st(y, 0, fp_reduce_once(fop_ld(x, 0)));
  else if constexpr (OP == FOP_REDUCE_2P) fop_st(y, 0, fp_reduce_2p(fop_ld(x, 0)));
  else if constexpr (OP == FOP_CANON3) fop_st(y, 0, fp_canon3(fop_ld(x, 0)));
  else if constexpr (OP == FOP_MUL) fop_st(y, 0, fp_mul(fop_ld(x, 0), fop_ld(x, 1)));
  else if constexpr (OP == FOP_SQR) fop_st(y, 0, fp_sqr(fop_ld(x, 0)));
  else if constexpr (OP == FOP_MUL_LAZY) fop_st(y, 0, fp_mul_lazy(fop_ld(x, 0), fop_ld(x, 1)));
  else if constexpr (OP == FOP_PREDS) y[0] = sf_preds(fop_ld(x, 0), fop_ld(x, 1));
#if defined(BLS_FP_D28)
  else if constexpr (OP == FOP_SQR_D28_LAZY) fop_st(y, 0, fp_sqr_d28_lazy(fop_ld(x, 0)));
  else if constexpr (OP == FOP_FP2_MUL_D28)
    fop_st2(y, 0, fp2_mul_d28(fop_ld(x, 0), fop_ld(x, 1), fop_ld(x, 2), fop_ld(x, 3)));
  else if constexpr (OP == FOP_FP2_SQR_D28) fop_st2(y, 0, fp2_sqr_d28(fop_ld(x, 0), fop_ld(x, 1)));
  else if constexpr (OP == FOP_FP2_MUL) fop_st2(y, 0, fp2_mul(fop_ld2(x, 0), fop_ld2(x, 1)));
  else if constexpr (OP == FOP_FP2_SQR) fop_st2(y, 0, fp2_sqr(fop_ld2(x, 0)));
  else if constexpr (OP == FOP_FP2_MUL_S) fop_st2(y, 0, fp2_mul_s(fop_ld2(x, 0), fop_ld2(x, 1)));
  else if constexpr (OP == FOP_LZ_MUL_RAW || OP == FOP_LZ_SQR_RAW) {
    Lz14 a, b;
#pragma unroll
    for (int k = 0; k < 14; ++k) {
      a.d[k] = (int32_t)x[k];
      b.d[k] = OP == FOP_LZ_MUL_RAW ? (int32_t)x[14 + k] : 0;
    }
    const Lz14 r = OP == FOP_LZ_MUL_RAW ? lz_mul_w(LZ_L14(a), LZ_L14(b)) : lz_sqr_w(LZ_L14(a));
#pragma unroll
    for (int k = 0; k < 14; ++k) y[k] = (uint32_t)r.d[k];
  } else if constexpr (OP == FOP_LZ_FP_OPS) {
    Fp r[10];
    sf_lz_fp_ops(fop_ld(x, 0), fop_ld(x, 1), r);
    for (int k = 0; k < 10; ++k) fop_st(y, k, r[k]);
  } else if constexpr (OP == FOP_LZ_FP2_OPS) {
    Fp2 r[6];
    sf_lz_fp2_ops(fop_ld2(x, 0), fop_ld2(x, 1), r);
    for (int k = 0; k < 6; ++k) fop_st2(y, k, r[k]);
  } else if constexpr (OP == FOP_INV) fop_st(y, 0, fp_inv(fop_ld(x, 0)));
  else if constexpr (OP == FOP_INV_GCD) fop_st(y, 0, fp_inv_gcd(fop_ld(x, 0)));
  else if constexpr (OP == FOP_SQRT) {
    Fp r = fp_zero();
    y[0] = fp_sqrt(fop_ld(x, 0), r) ? 1u : 0u;
    fop_st(y + 1, 0, r);
  } else if constexpr (OP == FOP_FP2_INV) fop_st2(y, 0, fp2_inv(fop_ld2(x, 0)));
  else if constexpr (OP == FOP_FP2_SQRT) {
    Fp2 r = fp2_zero();
    y[0] = fp2_sqrt(fop_ld2(x, 0), r) ? 1u : 0u;
    fop_st2(y + 1, 0, r);
  }
#if defined(__HIP_DEVICE_COMPILE__)  // the out-of-line primitives exist on the device only
  else if constexpr (OP == FOP_FP2_MUL_W) fop_st2(y, 0, fp2_mul_prim(fop_ld2(x, 0), fop_ld2(x, 1)));
  else if constexpr (OP == FOP_FP2_SQR_W) fop_st2(y, 0, fp2_sqr_prim(fop_ld2(x, 0)));
  else if constexpr (OP == FOP_FP2_CHAIN_W) {
    // a b, (a b) b, b (a b^2), (a b^3)(a b) = a^2 b^4: the slot takes b, b, a b^2, a b in turn
    const Fp2 a = fop_ld2(x, 0), b = fop_ld2(x, 1);
    const Fp2 r1 = fp2_mul_prim(a, b);
    const Fp2 r2 = fp2_mul_prim(r1, b);
    const Fp2 r3 = fp2_mul_prim(b, r2);
    fop_st2(y, 0, fp2_mul_prim(r3, r1));
  }
#endif
#endif
}

template <uint32_t OP, bool D28, int IN, int OUT>
__global__ __launch_bounds__(BLS_BLOCK) void k_field_op(const uint32_t* __restrict__ in, uint32_t n,
                                                        uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t x[IN], y[OUT];
#pragma unroll
  for (int k = 0; k < IN; ++k) x[k] = in[(size_t)IN * i + k];
#pragma unroll
  for (int k = 0; k < OUT; ++k) y[k] = 0;
  field_op_body<OP, D28>(x, y);
#pragma unroll
  for (int k = 0; k < OUT; ++k) out[(size_t)OUT * i + k] = y[k];
}

#if defined(BLS_FP_D28)
// "LIN8": the interpreter's linear combination (coop.hpp coop_lin) the way coop_step
// calls it.  Every lane stages its eight values in LDS slots 8 lane .. 8 lane + 7; term
// positions past the lane's n hold coefficient 0 and ref 0, as tools/gen_coop.py emit
// writes them; nmax is the wavefront's largest n, made wave-uniform with readfirstlane.
// Lanes past the last record take part with n = 0 (no early return before the barrier).
template <bool D28>
__global__ __launch_bounds__(BLS_BLOCK) void k_field_lin8(const uint32_t* __restrict__ in, uint32_t n,
                                                          uint32_t* __restrict__ out) {
  __shared__ Fp vals[BLS_BLOCK * 8];
  __shared__ int s_nmax;
  const uint32_t lane = threadIdx.x, i = blockIdx.x * BLS_BLOCK + lane;
  const bool live = i < n;
  if (lane == 0) s_nmax = 0;
  __syncthreads();
  uint16_t refs[8];
  int16_t cf[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    refs[k] = 0;
    cf[k] = 0;
  }
  int nt = 0;
  bool single = false;
  if (live) {
    const uint32_t* rec = in + (size_t)FOP_LIN8_IN * i;
    nt = rec[100] < 8u ? (int)rec[100] : 8;
    single = (rec[101] & 1u) != 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      lds_store_fp(vals, lane * 8 + k, fop_ld(rec, k));
      if (k < nt) {
        refs[k] = (uint16_t)(lane * 8 + k);
        cf[k] = (int16_t)(rec[96 + (k >> 1)] >> (16 * (k & 1)));
      }
    }
    atomicMax(&s_nmax, nt);
  }
  __syncthreads();
  const int nmax = __builtin_amdgcn_readfirstlane(s_nmax);
  const Fp r = coop_lin(refs, cf, nt, nmax, single, (const LdsU4*)vals);
  if (live) fop_st(out + 12ull * i, 0, r);
}
#endif

#define FOP_CASE(OP)                                                                                    \
  case OP:                                                                                              \
    k_field_op<OP, FOP_IS_D28, field_op_in_words(OP), field_op_out_words(OP)>                            \
        <<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(in, n, out);                                             \
    break

// launch base op `op` in this translation unit's flavour (in: n records of the op's
// in_words, out: n of its out_words); hipErrorInvalidValue for an op this flavour lacks
static hipError_t field_op_launch(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s) {
  switch (op) {
    FOP_CASE(FOP_ADD);
    FOP_CASE(FOP_SUB);
    FOP_CASE(FOP_NEG);
    FOP_CASE(FOP_DBL);
    FOP_CASE(FOP_HALF);
    FOP_CASE(FOP_ADD_NR);
    FOP_CASE(FOP_SUB_NR);
    FOP_CASE(FOP_REDUCE_ONCE);
    FOP_CASE(FOP_REDUCE_2P);
    FOP_CASE(FOP_MUL);
    FOP_CASE(FOP_SQR);
    FOP_CASE(FOP_MUL_LAZY);
    FOP_CASE(FOP_PREDS);
#if defined(BLS_FP_D28)
    FOP_CASE(FOP_CANON3);
    FOP_CASE(FOP_SQR_D28_LAZY);
    FOP_CASE(FOP_FP2_MUL_D28);
    FOP_CASE(FOP_FP2_SQR_D28);
    FOP_CASE(FOP_FP2_MUL);
    FOP_CASE(FOP_FP2_SQR);
    FOP_CASE(FOP_FP2_MUL_S);
    FOP_CASE(FOP_LZ_MUL_RAW);
    FOP_CASE(FOP_LZ_SQR_RAW);
    FOP_CASE(FOP_LZ_FP_OPS);
    FOP_CASE(FOP_LZ_FP2_OPS);
    FOP_CASE(FOP_INV);
    FOP_CASE(FOP_INV_GCD);
    FOP_CASE(FOP_SQRT);
    FOP_CASE(FOP_FP2_INV);
    FOP_CASE(FOP_FP2_SQRT);
    FOP_CASE(FOP_FP2_MUL_W);
    FOP_CASE(FOP_FP2_SQR_W);
    FOP_CASE(FOP_FP2_CHAIN_W);
    case FOP_LIN8:
      k_field_lin8<true><<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(in, n, out);
      break;
#endif
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bls
