// TEST INFRASTRUCTURE ONLY -- never linked into the product library.
//
// The fixed-base comb of the device pubkey table (bls/curve.hpp g1_comb_build /
// g1_comb_mul: what kernels/k_pk.hip k_comb_build and k_chain's role 3 run per lane)
// compiled for the host.  A stand-alone program (its own main), so it also runs under
// -fsanitize=address,undefined.
//
//   comb_host         self-check: for keys [k] g1 and scalars (a, b) -- random ones and the
//                     byte-column edge cases -- g1_comb_mul on the built rows equals
//                     jac_mul_glv in affine form, bit for bit; every row equals
//                     [sum bit_t(k) 2^(8t)] P by double-and-add; the infinity key and a key
//                     of order 3 report "no comb"; an on-curve key outside G1 either gives
//                     jac_mul_glv's element or reports "no comb".  Prints "ok <checks>"
//                     and exits 0, or the first mismatch and 1.
//   comb_host FILE    records of 104 bytes (96-byte uncompressed key, a and b as
//                     little-endian 32-bit words); one line per record:
//                       <status> <built 0|1> <comb96|-> <glv96> <15 rows, 96 bytes each|->
//                     (hex; status = g1_deserialize96's code, the rest "-" when it fails)
//                     for the caller to compare with the oracle (tests/test_comb_cpu.py).
#include <stdio.h>
#include <string.h>

#include <vector>

#define BLS_LAZY_POW 1
#include "bls/curve.hpp"

unsigned long long bls_fpm_counter = 0;
unsigned long long bls_lz_norm_counter = 0;

using namespace bls;

static int g_checks = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    ++g_checks;                                   \
    if (!(cond)) {                                \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
      return 1;                                   \
    }                                             \
  } while (0)

static uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static bool aff_eq(const G1A& a, const G1A& b) {
  if (a.inf || b.inf) return a.inf && b.inf;
  return fp_eq(a.x, b.x) && fp_eq(a.y, b.y);
}

static const uint32_t EDGE[6][2] = {{1u, 0u},          {0u, 1u},          {0xFFFFFFFFu, 0xFFFFFFFFu},
                                    {0x01010101u, 0u}, {0u, 0x80808080u}, {0x000000FFu, 0xFF000000u}};

static G1A glv_aff(const G1A& p, uint32_t a, uint32_t b) {
  G1J T[15];
  return jac_to_aff(jac_mul_glv<Fp>(jac_from_aff(p), a, b, T));
}

// rows against double-and-add, the comb against the GLV chain, for one key that builds
static int check_key(const G1A& p, uint64_t& seed, int n_random) {
  G1J T[G1_COMB_ROWS];
  Fp rows[G1_COMB_WORDS];
  CHECK(g1_comb_build(p, T, rows), "the builder refused a key of large order");
  for (uint32_t k = 1; k < 16; ++k) {
    uint64_t e = 0;
    for (int t = 0; t < 4; ++t)
      if ((k >> t) & 1u) e |= 1ull << (8 * t);
    G1A row;
    row.x = rows[2 * (k - 1)];
    row.y = rows[2 * (k - 1) + 1];
    row.inf = false;
    CHECK(g1_on_curve(row), "row %u is not on the curve", k);
    CHECK(aff_eq(row, jac_to_aff(aff_mul_u64(p, e))), "row %u != [%llx] P", k, (unsigned long long)e);
  }
  for (int s = 0; s < 6 + n_random; ++s) {
    uint32_t a, b;
    if (s < 6) a = EDGE[s][0], b = EDGE[s][1];
    else glv_split(splitmix(seed), a, b);
    const G1A want = glv_aff(p, a, b);
    const G1A got = jac_to_aff(g1_comb_mul(rows, a, b));
    CHECK(aff_eq(got, want), "comb != GLV for (a, b) = (%08x, %08x)", a, b);
  }
  return 0;
}

static int self_check() {
  uint64_t seed = 0x636f6d62ull;
  for (int k = 0; k < 32; ++k) {
    const G1A p = jac_to_aff(aff_mul_u64(g1_generator(), k < 2 ? 1ull + (uint64_t)k : splitmix(seed) | 1ull));
    if (check_key(p, seed, 8)) return 1;
  }
  G1J T[G1_COMB_ROWS];
  Fp rows[G1_COMB_WORDS];
  // the infinity key
  G1A inf;
  inf.x = fp_zero();
  inf.y = fp_zero();
  inf.inf = true;
  CHECK(!g1_comb_build(inf, T, rows), "the infinity key built a comb");
  // on-curve keys outside G1, not cofactor-cleared: (x, sqrt(x^3 + 4)) for the first small
  // x where that is a square.  x = 0 gives (0, 2), a point of order 3: [2^8] P = P, so the
  // entry P + [2^8] P + [2^16] P is infinity and the builder must refuse; the first x >= 1
  // has large order (its rows must then give the GLV chain's element).
  int seen_refused = 0, seen_equal = 0;
  for (uint32_t x0 = 0, found = 0; found < 2 && x0 < 64; ++x0) {
    G1A p;
    Fp xp = fp_zero();
    xp.l[0] = x0;
    p.x = fp_to_mont(xp);
    p.inf = false;
    if (!fp_sqrt(fp_add(fp_mul(fp_sqr(p.x), p.x), c_b1()), p.y)) continue;
    ++found;
    CHECK(g1_on_curve(p), "x = %u: not on the curve", x0);
    CHECK(!g1_in_subgroup(p), "x = %u: in G1 (cofactor h = 0x396c8c005555e1568c00aaab0000aaab)", x0);
    if (!g1_comb_build(p, T, rows)) {
      ++seen_refused;
      CHECK(x0 == 0, "x = %u: refused, but only the order-3 point should be", x0);
      continue;
    }
    ++seen_equal;
    uint64_t s2 = 0x6e6f6e4731ull + x0;
    for (int s = 0; s < 6 + 8; ++s) {
      uint32_t a, b;
      if (s < 6) a = EDGE[s][0], b = EDGE[s][1];
      else glv_split(splitmix(s2), a, b);
      CHECK(aff_eq(jac_to_aff(g1_comb_mul(rows, a, b)), glv_aff(p, a, b)),
            "x = %u outside G1: comb != GLV for (%08x, %08x)", x0, a, b);
    }
  }
  CHECK(seen_refused == 1 && seen_equal == 1, "outside G1: %d refused, %d equal (want 1 and 1)", seen_refused,
        seen_equal);
  printf("outside_g1 refused=%d equal=%d\n", seen_refused, seen_equal);
  printf("ok %d\n", g_checks);
  return 0;
}

static void put_hex(const uint8_t* b, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", b[i]);
}

static int run_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    printf("cannot open %s\n", path);
    return 2;
  }
  std::vector<uint8_t> rec(104);
  while (fread(rec.data(), 1, rec.size(), f) == rec.size()) {
    uint32_t a, b;
    memcpy(&a, rec.data() + 96, 4);
    memcpy(&b, rec.data() + 100, 4);
    G1A p;
    const int32_t code = g1_deserialize96(rec.data(), p);
    if (code != BLS_OK) {
      printf("%d 0 - - -\n", code);
      continue;
    }
    std::vector<G1J> T(G1_COMB_ROWS);
    std::vector<Fp> rows(G1_COMB_WORDS);
    const bool built = g1_comb_build(p, T.data(), rows.data());
    uint8_t out[96];
    printf("0 %d ", built ? 1 : 0);
    if (built) {
      g1_serialize96(jac_to_aff(g1_comb_mul(rows.data(), a, b)), out);
      put_hex(out, 96);
    } else {
      printf("-");
    }
    printf(" ");
    g1_serialize96(p.inf ? p : glv_aff(p, a, b), out);
    put_hex(out, 96);
    printf(" ");
    if (built) {
      for (int k = 0; k < G1_COMB_ROWS; ++k) {
        G1A row;
        row.x = rows[2 * k];
        row.y = rows[2 * k + 1];
        row.inf = false;
        g1_serialize96(row, out);
        put_hex(out, 96);
      }
    } else {
      printf("-");
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) { return argc > 1 ? run_file(argv[1]) : self_check(); }
