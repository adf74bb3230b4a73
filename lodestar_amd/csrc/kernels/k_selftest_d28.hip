// Field-op self-test kernels over the 28-bit-digit Montgomery product (BLS_FP_D28, as
// k_pre, k_chain, the Miller loops, k_pset, k_fin and the MSM build it): the primitives
// the verify path executes, one per launch, on raw operands (kernels/field_ops.hpp).
#define BLS_FP_D28 1
#include "../launchers.hpp"
#include "field_ops.hpp"
#include "curve_ops.hpp"
#include "tower_ops.hpp"

using namespace bls;

hipError_t launch_k_field_op_d28(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s) {
  return field_op_launch(op, in, n, out, s);
}

hipError_t launch_k_curve_op_d28(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s) {
  return curve_op_launch(op, in, n, out, s);
}

hipError_t launch_k_tower_op_d28(uint32_t op, const Fp* in, uint32_t n, Fp* out, hipStream_t s) {
  return tower_op_launch(op, in, n, out, s);
}
