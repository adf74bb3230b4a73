// Formula bodies of the lazy28 and predicate self-tests, shared by the CPU harness
// (tests/native/hostsim.cpp hs_lz_fp_ops / hs_lz_fp2_ops) and the device field-op
// self-test (kernels/field_ops.hpp): the same expressions run on both, on canonical
// Montgomery operands, and return canonical Montgomery values.
#pragma once

#include "field.hpp"

namespace bls {

// ten values (tests/_fieldvec.py lz_fp_ref): a b, a^2, a + b, a - b, -(a b), a b / 2,
// -(a b) through lz_norm, (2ab - b^2)(b - a), a (round trip), 4 (2ab - 7 b^2 - 7 a)
// through lz_reduce; a lz_reduce digit out of [0, 2^28) flips out[0]'s low limb
BLS_HD void sf_lz_fp_ops(const Fp& a, const Fp& b, Fp out[10]) {
  const auto x = lz_from_fp(a), y = lz_from_fp(b);
  const auto xy = lz_mul(x, y);
  out[0] = lz_to_fp(xy);
  out[1] = lz_to_fp(lz_sqr(x));
  out[2] = lz_to_fp(lz_add(x, y));
  out[3] = lz_to_fp(lz_sub(x, y));
  out[4] = lz_to_fp(lz_neg(xy));
  out[5] = lz_to_fp(lz_half(xy));
  out[6] = lz_to_fp(lz_norm(lz_sub(xy, lz_dbl(xy))));
  const auto s = lz_sub(lz_add(xy, xy), lz_mul(y, y));
  out[7] = lz_to_fp(lz_mul(s, lz_norm(lz_sub(y, x))));
  out[8] = lz_to_fp(x);
  // lz_reduce of a large signed combination (|value| up to 128 p)
  const auto big = lz_sub(lz_sub(lz_add(xy, xy), lz_mulc<7>(lz_mul(y, y))), lz_mulc<7>(lz_mul(x, lz_one())));
  const auto red = lz_reduce(lz_add(lz_add(big, big), lz_add(big, big)));
  out[9] = lz_to_fp(red);
  for (int k = 0; k < 13; ++k)
    if (red.d[k] < 0 || red.d[k] > (int32_t)LZ_M28) out[0].l[0] ^= 0xFFu;  // digits normalised
}

// six Fp2 values: mul, sqr, mul_xi(mul), conj(mul), mul - b^2, mul * b.c0
BLS_HD void sf_lz_fp2_ops(const Fp2& a, const Fp2& b, Fp2 out[6]) {
  const auto x = l2_from_fp2(a), y = l2_from_fp2(b);
  const auto m = l2_mul(x, y);
  out[0] = l2_to_fp2(m);
  out[1] = l2_to_fp2(l2_sqr(x));
  out[2] = l2_to_fp2(l2_mul_xi(m));
  out[3] = l2_to_fp2(l2_conj(m));
  out[4] = l2_to_fp2(l2_sub(m, l2_sqr(y)));
  out[5] = l2_to_fp2(l2_mul_fp(m, y.c0));
}

// "PREDS": every comparison predicate of field.hpp on one raw pair (c0, c1), one bit each
// (tests/_fieldvec.py PRED_BITS).  Bits 0..6 read the words as plain values and are
// defined on any 384-bit input; bits 7..11 read them as Montgomery forms and are
// defined on canonical input only.
BLS_HD uint32_t sf_preds(const Fp& c0, const Fp& c1) {
  const Fp2 a{c0, c1};
  uint32_t r = 0;
  r |= fp_plain_is_canonical(c0) ? 1u << 0 : 0u;
  r |= fp_plain_is_canonical(c1) ? 1u << 1 : 0u;
  r |= fp_plain_gt_half(c0) ? 1u << 2 : 0u;
  r |= fp_plain_gt_half(c1) ? 1u << 3 : 0u;
  r |= fp_is_zero(c0) ? 1u << 4 : 0u;
  r |= fp_is_zero(c1) ? 1u << 5 : 0u;
  r |= fp_eq(c0, c1) ? 1u << 6 : 0u;
  r |= fp_lex_largest(c0) ? 1u << 7 : 0u;
  r |= fp_lex_largest(c1) ? 1u << 8 : 0u;
  r |= fp2_lex_largest(a) ? 1u << 9 : 0u;
  r |= (fp2_sgn0(a) & 1u) << 10;
  r |= fp2_is_zero(a) ? 1u << 11 : 0u;
  return r;
}

}  // namespace bls
