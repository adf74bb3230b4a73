// Field self-test and Fp-product probes: canonical-byte Fp products (parity against
// the oracle) and a dependent chain of Montgomery products per lane (latency when
// one wave runs alone, throughput when every CU is busy).
#include "../launchers.hpp"
#include "field_ops.hpp"
#include "curve_ops.hpp"
#include "tower_ops.hpp"

using namespace bls;

__global__ __launch_bounds__(BLS_BLOCK) void k_fp_mul_test(const uint8_t* a, const uint8_t* b, uint32_t n,
                                                           uint8_t* out) {
  uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i >= n) return;
  Fp x = fp_to_mont(fp_from_be48(a + 48ull * i));
  Fp y = fp_to_mont(fp_from_be48(b + 48ull * i));
  // equal operands go through the dedicated squaring
  fp_to_be48(fp_from_mont(fp_eq(x, y) ? fp_sqr(x) : fp_mul(x, y)), out + 48ull * i);
}

__global__ __launch_bounds__(BLS_BLOCK) void k_fpm_chain(Fp* io, uint32_t iters) {
  uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  Fp a = io[2 * i], b = io[2 * i + 1];
  for (uint32_t k = 0; k < iters; ++k) a = fp_mul(a, b);
  io[2 * i] = a;
}

hipError_t launch_k_fp_mul_test(const uint8_t* a, const uint8_t* b, uint32_t n, uint8_t* out, hipStream_t s) {
  k_fp_mul_test<<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(a, b, n, out);
  return hipGetLastError();
}
hipError_t launch_k_fpm_chain(Fp* io, uint32_t lanes, uint32_t iters, hipStream_t s) {
  k_fpm_chain<<<lanes / BLS_BLOCK, BLS_BLOCK, 0, s>>>(io, iters);
  return hipGetLastError();
}

// the field-op self-test: this translation unit's kernels run the 32-bit column product,
// kernels/k_selftest_d28.hip's the 28-bit-digit one (op bit FOP_D28_FLAG)
int field_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words) {
  const uint32_t base = op & ~FOP_D28_FLAG;
  if (base >= FOP_COUNT || (field_op_d28_only(base) && !(op & FOP_D28_FLAG))) return -2;
  if (in_words) *in_words = (uint32_t)field_op_in_words(base);
  if (out_words) *out_words = (uint32_t)field_op_out_words(base);
  return 0;
}
hipError_t launch_k_field_op(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s) {
  if (field_op_shape(op, nullptr, nullptr) != 0) return hipErrorInvalidValue;
  if (op & FOP_D28_FLAG) return launch_k_field_op_d28(op & ~FOP_D28_FLAG, in, n, out, s);
  return field_op_launch(op, in, n, out, s);
}

// the curve-op self-test (kernels/curve_ops.hpp): the 32-bit column flavour here, the
// 28-bit-digit one in kernels/k_selftest_d28.hip, iso_jac_nl and chain_role_h beside
// k_chain in kernels/k_chain.hip
int curve_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words) {
  const uint32_t base = op & ~COP_D28_FLAG;
  if (base >= COP_COUNT || !(curve_op_flavours(base) & ((op & COP_D28_FLAG) ? 2u : 1u))) return -2;
  if (in_words) *in_words = (uint32_t)curve_op_in_words(base);
  if (out_words) *out_words = (uint32_t)curve_op_out_words(base);
  return 0;
}
size_t curve_op_ws_bytes(uint32_t op, uint32_t n) {
  return (op & ~COP_D28_FLAG) == COP_CHAIN_H ? (sizeof(Fp) * CHAIN_WORDS + 4u) * (size_t)n : 0;
}
hipError_t launch_k_curve_op(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, void* ws, hipStream_t s) {
  const uint32_t base = op & ~COP_D28_FLAG;
  if (curve_op_shape(op, nullptr, nullptr) != 0 || curve_op_on_host(base)) return hipErrorInvalidValue;
  if (curve_op_in_chain_tu(base)) return launch_k_curve_op_chain(base, in, n, out, ws, s);
  if (op & COP_D28_FLAG) return launch_k_curve_op_d28(base, in, n, out, s);
  return curve_op_launch(base, in, n, out, s);
}

// the tower-op self-test (kernels/tower_ops.hpp): the 32-bit column flavour here, the
// 28-bit-digit one in kernels/k_selftest_d28.hip, the file-local functions of
// kernels/k_fin_simt.hip and kernels/k_mlq.hip beside the kernels that call them
int tower_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words) {
  const uint32_t base = op & ~TOP_D28_FLAG;
  if (base >= TOP_COUNT || !(tower_op_flavours(base) & ((op & TOP_D28_FLAG) ? 2u : 1u))) return -2;
  if (in_words) *in_words = 12u * (uint32_t)tower_op_in_fps(base);
  if (out_words) *out_words = 12u * (uint32_t)tower_op_out_fps(base);
  return 0;
}
hipError_t launch_k_tower_op(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s) {
  const uint32_t base = op & ~TOP_D28_FLAG;
  if (tower_op_shape(op, nullptr, nullptr) != 0 || tower_op_on_host(base)) return hipErrorInvalidValue;
  const Fp* fin = reinterpret_cast<const Fp*>(in);
  Fp* fout = reinterpret_cast<Fp*>(out);
  if (tower_op_in_fin_tu(base)) return launch_k_tower_op_fin(base, fin, n, fout, s);
  if (tower_op_in_mlq_tu(base)) return launch_k_tower_op_mlq(base, fin, n, fout, s);
  if (op & TOP_D28_FLAG) return launch_k_tower_op_d28(base, fin, n, fout, s);
  return tower_op_launch(base, fin, n, fout, s);
}
