// TEST INFRASTRUCTURE ONLY -- never linked into the product library.
//
// CPU build of the row-wise lazy Fp2 product and square (bls/field.hpp fp2_mul_rows /
// fp2_sqr_rows, the bodies of the device's out-of-line fp2_mul_w / fp2_sqr_w) on raw
// little-endian limbs: Montgomery form in and out, coefficients up to the stated input
// bound (< 2p).  tests: tests/test_fp2_bound.py.
#include <string.h>

#include "bls/field.hpp"

using namespace bls;

extern "C" {

// a = a0 | a1, b = b0 | b1 (48 bytes each), out = c0 | c1
void fr_fp2_mul_rows_raw(const uint8_t* a, const uint8_t* b, uint8_t* out) {
  Fp a0, a1, b0, b1;
  memcpy(a0.l, a, 48);
  memcpy(a1.l, a + 48, 48);
  memcpy(b0.l, b, 48);
  memcpy(b1.l, b + 48, 48);
  const Fp2 r = fp2_mul_rows(a0, a1, b0, b1);
  memcpy(out, r.c0.l, 48);
  memcpy(out + 48, r.c1.l, 48);
}

void fr_fp2_sqr_rows_raw(const uint8_t* a, uint8_t* out) {
  Fp a0, a1;
  memcpy(a0.l, a, 48);
  memcpy(a1.l, a + 48, 48);
  const Fp2 r = fp2_sqr_rows(a0, a1);
  memcpy(out, r.c0.l, 48);
  memcpy(out + 48, r.c1.l, 48);
}

}  // extern "C"
