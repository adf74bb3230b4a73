// The span rules of bls/committee.hpp on the CPU (what bls_gpu_verify_spans,
// bls_gpu_aggregate_spans, k_pk_span and the verifiers' routing weight share): the bit
// accessor at a bit offset, the length and padding check over the sum of the segments'
// sizes, span_weight, every -2 case of span_check_sets with its message, and the single-lane
// statement span_select_sum over integers standing in for points -- it must equal the plain
// sum over the set bits of the concatenation, and read exactly sum_k min(c_k, n_k - c_k)
// members (one more for a segment at the tie c == n - c + 1, which stays direct), the
// complement taken exactly when committee_use_complement says so.
// Stand-alone: prints "ok <checks>" and exits 0, or says what failed and exits 1.  Built
// plain and with -fsanitize=address,undefined by tests/test_span_cpu.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bls/committee.hpp"

using namespace bls;

namespace {

long g_checks = 0;
int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      if (!g_failed++) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

typedef unsigned long long Z;
Z key_at(uint32_t i) { return 1000003ull * i + 17ull; }

// exact-size heap copies, so that a read one byte past a field is the sanitizer's to see
struct Field {
  uint8_t* p;
  uint32_t n_bytes;
  explicit Field(const std::vector<uint8_t>& v) : p((uint8_t*)malloc(v.size() ? v.size() : 1)), n_bytes((uint32_t)v.size()) {
    if (!v.empty()) memcpy(p, v.data(), v.size());
  }
  ~Field() { free(p); }
  Field(const Field&) = delete;
  Field& operator=(const Field&) = delete;
};

void set_bit(std::vector<uint8_t>& f, uint32_t j) { f[j >> 3] |= (uint8_t)(1u << (j & 7)); }

void test_bits() {
  // the accessor at a bit offset: segment k's bit j is bit off_k + j of the field
  for (uint32_t off : {0u, 1u, 7u, 8u, 9u, 63u, 64u, 65u}) {
    for (uint32_t n : {1u, 7u, 8u, 9u, 65u}) {
      std::vector<uint8_t> f(committee_bits_bytes(off + n), 0);
      for (uint32_t j = 0; j < n; j += 2) set_bit(f, off + j);
      if (off) set_bit(f, off - 1);  // the previous segment's last bit is not this one's
      const Field h(f);
      for (uint32_t j = 0; j < n; ++j) {
        CHECK(span_bit(h.p, off, j) == ((j & 1) == 0));
        CHECK(span_selects(h.p, off, j, false) == ((j & 1) == 0));
        CHECK(span_selects(h.p, off, j, true) == ((j & 1) == 1));
      }
      CHECK(span_popcount(h.p, off, n) == (n + 1) / 2);
    }
  }
  // length and padding over the sum of the sizes, however it is cut into segments
  struct Cut {
    uint32_t total;
    std::vector<uint32_t> seg;
  };
  const std::vector<Cut> cuts = {{8, {8}},       {8, {1, 7}},      {8, {3, 5}},        {9, {9}},          {9, {8, 1}},
                                 {9, {1, 1, 7}}, {16, {7, 9}},     {16, {8, 8}},       {17, {9, 8}},      {17, {1, 7, 9}},
                                 {64, {63, 1}},  {64, {1, 7, 56}}, {65, {64, 1}},      {65, {9, 56}},     {65, {65}}};
  for (const Cut& cut : cuts) {
    const uint32_t total = span_members(cut.seg.data(), (uint32_t)cut.seg.size());
    CHECK(total == cut.total);
    const uint32_t nb = committee_bits_bytes(total);
    CHECK(nb == (total + 7) / 8);
    {
      const Field z(std::vector<uint8_t>(nb + 1, 0));
      CHECK(span_check_bits(z.p, nb, total) == BLS_CODE_OK);
      CHECK(span_check_bits(z.p, nb + 1, total) == BLS_CODE_BAD_ENCODING);  // one byte long
      CHECK(span_check_bits(z.p, nb - 1, total) == BLS_CODE_BAD_ENCODING);  // one byte short
      CHECK(span_check_bits(z.p, 0, total) == BLS_CODE_BAD_ENCODING);
    }
    for (uint32_t j = 0; j < 8 * nb; ++j) {
      std::vector<uint8_t> f(nb, 0);
      set_bit(f, j);
      const Field h(f);
      CHECK(span_check_bits(h.p, nb, total) == (j < total ? BLS_CODE_OK : BLS_CODE_BAD_ENCODING));
      if (j >= total) continue;
      // the bit belongs to exactly one segment, at its own offset
      uint32_t off = 0, owners = 0;
      for (uint32_t n : cut.seg) {
        const uint32_t c = span_popcount(h.p, off, n);
        owners += c;
        if (c) CHECK(j >= off && j < off + n && span_bit(h.p, off, j - off));
        off += n;
      }
      CHECK(owners == 1);
    }
    const Field ones(std::vector<uint8_t>(nb, 0xFF));
    CHECK(span_check_bits(ones.p, nb, total) == ((total & 7) ? BLS_CODE_BAD_ENCODING : BLS_CODE_OK));
  }
}

void test_weight() {
  const uint32_t n1[1] = {512}, c1[1] = {507};
  CHECK(span_weight(n1, c1, 1) == committee_weight(512, 507) && span_weight(n1, c1, 1) == 6);
  const uint32_t n3[3] = {512, 8, 9}, c3[3] = {5, 4, 0};
  CHECK(span_weight(n3, c3, 3) == 6 + 5 + 1);
  CHECK(span_weight(n3, c3, 0) == 0);
  // a mainnet attestation: 64 committees of 500, 5 absent in each
  std::vector<uint32_t> n(64, 500), c(64, 495);
  CHECK(span_weight(n.data(), c.data(), 64) == 64 * 6);
  uint32_t w = 0;
  for (uint32_t k = 0; k < 64; ++k) {
    n[k] = 1 + 7 * (k & 1);
    c[k] = k % (n[k] + 1);
    w += committee_weight(n[k], c[k]);
  }
  CHECK(span_weight(n.data(), c.data(), 64) == w);
}

int expect(const bls_span_sets* ss, uint32_t n_sets, bool in_batch, const uint32_t* po, const char* want) {
  char err[256] = "";
  const int rc = span_check_sets(ss, n_sets, in_batch, po, err, sizeof(err));
  if (want) {
    CHECK(rc == -2);
    CHECK(strstr(err, want) != nullptr);
    if (!strstr(err, want)) fprintf(stderr, "  message was: %s (wanted \"%s\")\n", err, want);
  } else {
    CHECK(rc == 0);
    CHECK(err[0] == 0);
    if (err[0]) fprintf(stderr, "  unexpected message: %s\n", err);
  }
  return rc;
}

void test_check_sets() {
  // set 0: two segments; set 1: an index list; set 2: one segment
  const uint32_t so[4] = {0, 2, 2, 3};
  const uint32_t refs[3] = {BLS_COMMITTEE_REF(1, 2), BLS_COMMITTEE_REF(0, 0), BLS_COMMITTEE_REF(1, 2)};
  const uint32_t bo[4] = {0, 2, 2, 3};
  const uint32_t po[4] = {0, 0, 3, 3};
  const uint8_t bits[3] = {1, 2, 3};
  const bls_span_sets good = {so, refs, bo, bits};
  expect(&good, 3, true, po, nullptr);
  expect(&good, 0, true, nullptr, nullptr);
  expect(&good, 0, false, nullptr, nullptr);

  // a NULL array where one is needed
  expect(nullptr, 3, true, po, "set_span_off or set_bits_off missing");
  expect(nullptr, 0, true, po, "missing");
  bls_span_sets ss = good;
  ss.set_span_off = nullptr;
  expect(&ss, 3, true, po, "set_span_off or set_bits_off missing");
  ss = good;
  ss.set_bits_off = nullptr;
  expect(&ss, 3, true, po, "set_span_off or set_bits_off missing");
  ss = good;
  ss.span_refs = nullptr;
  expect(&ss, 3, true, po, "span_refs missing");
  ss = good;
  ss.bits = nullptr;
  expect(&ss, 3, true, po, "bits missing");
  // a raw-key batch
  expect(&good, 3, true, nullptr, "raw keys");

  // offsets that do not run monotonically from 0
  const uint32_t so_first[4] = {1, 2, 2, 3};
  ss = good;
  ss.set_span_off = so_first;
  expect(&ss, 3, true, po, "set_span_off[0] != 0");
  const uint32_t bo_first[4] = {1, 2, 2, 3};
  ss = good;
  ss.set_bits_off = bo_first;
  expect(&ss, 3, true, po, "set_bits_off[0] != 0");
  const uint32_t so_back[4] = {0, 2, 1, 3};
  ss = good;
  ss.set_span_off = so_back;
  expect(&ss, 3, true, po, "set_span_off not monotone at set 1");
  const uint32_t bo_back[4] = {0, 2, 1, 3};
  ss = good;
  ss.set_bits_off = bo_back;
  expect(&ss, 3, true, po, "set_bits_off not monotone at set 1");

  // a span set that also carries an index list; an index-list set that carries bits
  const uint32_t po_list[4] = {0, 0, 3, 4};
  expect(&good, 3, true, po_list, "set 2 is a span and carries an index list");
  const uint32_t bo_no[4] = {0, 2, 3, 3};
  ss = good;
  ss.set_bits_off = bo_no;
  expect(&ss, 3, true, po, "set 1 has no segment and carries 1 bytes of bits");

  // the cap: exactly BLS_SPAN_MAX_COMMITTEES segments pass, one more does not
  std::vector<uint32_t> many(2 * BLS_SPAN_MAX_COMMITTEES + 1, BLS_COMMITTEE_REF(0, 0));
  const uint32_t so_cap[3] = {0, BLS_SPAN_MAX_COMMITTEES, 2 * BLS_SPAN_MAX_COMMITTEES + 1};
  const uint32_t bo2[3] = {0, 1, 3};
  const uint32_t po2[3] = {0, 0, 0};
  const bls_span_sets cap = {so_cap, many.data(), bo2, bits};
  expect(&cap, 1, true, po2, nullptr);
  expect(&cap, 2, true, po2, "set 1 has 65 segments, the cap is 64");
  expect(&cap, 2, false, nullptr, "set 1 has 65 segments");

  // the aggregate call: no batch beside it, and every set needs a segment
  const uint32_t so_all[4] = {0, 2, 2, 3};
  expect(&good, 1, false, nullptr, nullptr);
  ss = good;
  ss.set_span_off = so_all;
  expect(&ss, 3, false, nullptr, "set 1 has no segment");
  CHECK(BLS_SPAN_MAX_COMMITTEES == 64u);
}

// the single-lane statement over integers
struct Committee {
  std::vector<uint32_t> mem;
  Z total;
};

void test_selection() {
  uint32_t seed = 2718281;
  const auto rnd = [&]() { return seed = seed * 1664525u + 1013904223u; };
  long reads = 0;
  const auto at = [&](uint32_t m) {
    ++reads;
    return key_at(m);
  };
  const auto add = [](Z a, Z b) { return a + b; };
  const auto neg = [](Z a) { return (Z)0 - a; };

  std::vector<Committee> cm;
  for (uint32_t n : {1u, 7u, 8u, 9u, 63u, 64u, 65u, 129u}) {
    Committee c;
    c.total = 0;
    for (uint32_t j = 0; j < n; ++j) {
      c.mem.push_back(rnd() % 109);  // duplicates within and across committees on purpose
      c.total += key_at(c.mem.back());
    }
    cm.push_back(c);
  }
  const auto by_size = [&](uint32_t n) -> uint32_t {
    for (uint32_t k = 0; k < cm.size(); ++k)
      if (cm[k].mem.size() == n) return k;
    abort();
  };
  std::vector<std::vector<uint32_t>> spans = {{7, 9}, {1, 1, 1}, {9, 63, 65}, {65, 64, 1}, {129, 7, 129}, {8, 8}, {9, 9}, {64}};
  {
    std::vector<uint32_t> cap;
    for (uint32_t k = 0; k < BLS_SPAN_MAX_COMMITTEES; ++k) cap.push_back((k & 1) ? 7u : 1u);
    spans.push_back(cap);
  }
  // per segment: all, all-but-first, all-but-last, first-only, last-only, none, half, random
  const int N_PAT = 8;
  const auto pattern = [&](int which, uint32_t n, uint32_t j) -> bool {
    switch (which) {
      case 0: return true;
      case 1: return j != 0;
      case 2: return j != n - 1;
      case 3: return j == 0;
      case 4: return j == n - 1;
      case 5: return false;
      case 6: return j < n / 2;
      default: return rnd() % 100 < 80;
    }
  };
  long direct = 0, complement = 0, mixed_sets = 0;
  for (const auto& sizes : spans) {
    const uint32_t n_seg = (uint32_t)sizes.size();
    std::vector<const uint32_t*> mem(n_seg);
    std::vector<uint32_t> seg_n(n_seg);
    std::vector<Z> tot(n_seg);
    for (uint32_t k = 0; k < n_seg; ++k) {
      const Committee& c = cm[by_size(sizes[k])];
      mem[k] = c.mem.data();
      seg_n[k] = sizes[k];
      tot[k] = c.total;
    }
    const uint32_t total = span_members(seg_n.data(), n_seg), nb = committee_bits_bytes(total);
    // every combination of patterns for up to three segments; a rotating choice beyond that
    const long combos = n_seg <= 3 ? (n_seg == 1 ? N_PAT : n_seg == 2 ? N_PAT * N_PAT : N_PAT * N_PAT * N_PAT) : 4 * N_PAT;
    for (long combo = 0; combo < combos; ++combo) {
      std::vector<uint8_t> f(nb, 0);
      std::vector<uint32_t> seg_c(n_seg, 0);
      Z want = 0;
      uint32_t off = 0;
      for (uint32_t k = 0; k < n_seg; ++k) {
        long which = n_seg <= 3 ? (combo / (k == 0 ? 1 : k == 1 ? N_PAT : N_PAT * N_PAT)) % N_PAT : (combo + 3 * k + combo / N_PAT * k) % N_PAT;
        for (uint32_t j = 0; j < seg_n[k]; ++j)
          if (pattern((int)which, seg_n[k], j)) {
            set_bit(f, off + j);
            want += key_at(mem[k][j]);
            ++seg_c[k];
          }
        off += seg_n[k];
      }
      const Field h(f);
      CHECK(span_check_bits(h.p, h.n_bytes, total) == BLS_CODE_OK);
      long want_reads = 0, n_comp = 0, min_reads = 0, ties = 0;
      off = 0;
      for (uint32_t k = 0; k < n_seg; ++k) {
        CHECK(span_popcount(h.p, off, seg_n[k]) == seg_c[k]);
        const bool comp = committee_use_complement(seg_n[k], seg_c[k]);
        want_reads += comp ? seg_n[k] - seg_c[k] : seg_c[k];
        // min(c, n - c) members, but for the tie c == n - c + 1: there the complement would cost
        // as many additions (its n - c members and the total), so the set bits are read
        const uint32_t least = seg_c[k] < seg_n[k] - seg_c[k] ? seg_c[k] : seg_n[k] - seg_c[k];
        const bool tie = seg_c[k] == seg_n[k] - seg_c[k] + 1;
        CHECK((comp ? seg_n[k] - seg_c[k] : seg_c[k]) == least + (tie ? 1u : 0u));
        CHECK(!(tie && comp));
        min_reads += least;
        ties += tie;
        n_comp += comp;
        (comp ? complement : direct)++;
        off += seg_n[k];
      }
      if (n_comp && n_comp < (long)n_seg) ++mixed_sets;
      reads = 0;
      const Z got = span_select_sum<Z>(mem.data(), seg_n.data(), tot.data(), n_seg, h.p, (Z)0, true, at, add, neg);
      CHECK(got == want);
      CHECK(reads == want_reads);
      CHECK(reads == min_reads + ties);
      CHECK(span_weight(seg_n.data(), seg_c.data(), n_seg) == (uint32_t)min_reads + n_seg);
      reads = 0;
      const Z plain = span_select_sum<Z>(mem.data(), seg_n.data(), tot.data(), n_seg, h.p, (Z)0, false, at, add, neg);
      CHECK(plain == want);
      long set_bits = 0;
      for (uint32_t c : seg_c) set_bits += c;
      CHECK(reads == set_bits);
      // a wrong total of segment k shows exactly when segment k is complemented
      for (uint32_t k = 0; k < n_seg && k < 3; ++k) {
        std::vector<Z> t2 = tot;
        t2[k] += 1;
        const Z off_by = span_select_sum<Z>(mem.data(), seg_n.data(), t2.data(), n_seg, h.p, (Z)0, true, at, add, neg);
        CHECK((off_by != want) == committee_use_complement(seg_n[k], seg_c[k]));
      }
      // one segment: the committee rule itself
      if (n_seg == 1) {
        const Z one = committee_select_sum<Z>(mem[0], seg_n[0], h.p, tot[0], (Z)0, true, at, add, neg);
        CHECK(one == got);
      }
    }
  }
  CHECK(direct > 100 && complement > 100 && mixed_sets > 50);
}

}  // namespace

int main() {
  test_bits();
  test_weight();
  test_check_sets();
  test_selection();
  if (g_failed) {
    fprintf(stderr, "span_host: %d checks failed\n", g_failed);
    return 1;
  }
  printf("ok %ld\n", g_checks);
  return 0;
}
