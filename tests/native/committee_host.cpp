// bls/committee.hpp on the CPU: the argument validation of a registration case by case, the
// group slots over a counting allocator (set / replace / drop / close: every allocation freed
// exactly once, the byte accounting as bls_gpu_committee_group_info reports it), and the
// selection rules -- the complement decision at its tie, the length and padding checks, and
// the single-lane statement of the kernel's sum over integers standing in for points, where
// the direct and the complement branch must both give the direct sum.  Stand-alone: prints
// "ok <checks>" and exits 0, or says what failed and exits 1.  Built plain and with
// -fsanitize=address,undefined by tests/test_committee_cpu.py.
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

// ---- the allocator: counts, remembers what is live, refuses on request
struct Block {
  uint8_t* p;
  size_t bytes;
  bool live;
};
std::vector<Block> g_heap;
long g_allocs = 0, g_frees = 0;
bool g_fail_next = false;

void* h_alloc(size_t bytes) {
  if (g_fail_next) {
    g_fail_next = false;
    return nullptr;
  }
  uint8_t* p = (uint8_t*)malloc(bytes);
  memset(p, 0xA5, bytes);
  g_heap.push_back(Block{p, bytes, true});
  ++g_allocs;
  return p;
}
void h_free(void* p) {
  bool found = false;
  for (Block& b : g_heap)
    if (b.p == p && b.live) {
      b.live = false;
      found = true;
      free(b.p);
      break;
    }
  CHECK(found);  // neither a double free nor a pointer that was never handed out
  ++g_frees;
}
bool h_copy(void* dst, const void* src, size_t bytes, void*) {
  memcpy(dst, src, bytes);
  return true;
}
bool h_sync(void*) { return true; }
const PkMem MEM = {h_alloc, h_free, h_copy, h_sync};

long live_blocks() {
  long n = 0;
  for (const Block& b : g_heap) n += b.live;
  return n;
}
size_t live_bytes() {
  size_t n = 0;
  for (const Block& b : g_heap) n += b.live ? b.bytes : 0;
  return n;
}

// integers stand in for points: key i is the value 1000003 i + 17 (mod 2^64)
typedef unsigned long long Z;
Z key_at(uint32_t i) { return 1000003ull * i + 17ull; }
constexpr size_t TOTAL_BYTES = sizeof(Z);

bool upload(void* dst, const void* src, size_t bytes) {
  memcpy(dst, src, bytes);
  return true;
}
bool g_fail_totals = false;
bool totals(const CommitteeGroupDev& v) {
  if (g_fail_totals) return false;
  Z* t = (Z*)v.totals;
  for (uint32_t c = 0; c < v.n; ++c) {
    Z sum = 0;
    for (uint32_t k = v.offsets[c]; k < v.offsets[c + 1]; ++k) sum += key_at(v.members[k]);
    t[c] = sum;
  }
  return true;
}

int check(uint32_t group, uint32_t n, const std::vector<uint32_t>& off, const std::vector<uint32_t>& mem,
          uint32_t table_n, const char* expect) {
  char err[256] = "";
  const int rc = committee_check_group(group, n, off.data(), mem.data(), table_n, err, sizeof(err));
  if (expect) {
    CHECK(rc == -2);
    CHECK(strstr(err, expect) != nullptr);
    if (!strstr(err, expect)) fprintf(stderr, "  message was: %s (wanted \"%s\")\n", err, expect);
  } else {
    CHECK(rc == 0);
    CHECK(err[0] == 0);
  }
  return rc;
}

void test_validation() {
  const std::vector<uint32_t> off = {0, 3, 4, 8}, mem = {0, 1, 2, 9, 4, 4, 5, 6};
  check(0, 3, off, mem, 10, nullptr);
  check(7, 3, off, mem, 10, nullptr);
  check(8, 3, off, mem, 10, "group 8");
  check(8, 0, off, mem, 10, "group 8");  // a drop of a slot that does not exist
  check(3, 0, {}, {}, 0, nullptr);       // a drop needs no arrays
  // a member at the table's size (the last valid index is 9), named with its committee
  check(1, 3, off, mem, 9, "committee 1 member 0 is table index 9");
  check(1, 3, off, {0, 1, 2, 3, 4, 4, 5, 0xFFFFFFFFu}, 10, "committee 2 member 3");
  check(1, 3, {0, 3, 3, 8}, mem, 10, "committee 1 is empty");
  check(1, 3, {0, 0, 4, 8}, mem, 10, "committee 0 is empty");
  check(1, 3, {0, 5, 4, 8}, mem, 10, "not monotone at committee 1");
  check(1, 3, {1, 3, 4, 8}, mem, 10, "member_offsets[0] != 0");
  {
    char err[128] = "";
    CHECK(committee_check_group(0, 2, nullptr, mem.data(), 10, err, sizeof(err)) == -2);
    CHECK(committee_check_group(0, 2, off.data(), nullptr, 10, err, sizeof(err)) == -2);
  }
  // the cap: exactly BLS_COMMITTEE_MAX_MEMBERS passes, one more does not
  std::vector<uint32_t> big(BLS_COMMITTEE_MAX_MEMBERS + 1u, 0u);
  check(0, 1, {0, BLS_COMMITTEE_MAX_MEMBERS}, big, 1, nullptr);
  check(0, 2, {0, 1, BLS_COMMITTEE_MAX_MEMBERS + 2u}, std::vector<uint32_t>(BLS_COMMITTEE_MAX_MEMBERS + 2u, 0u), 1,
        "committee 1 has 131073 members");
  // duplicates are members like any other
  check(0, 1, {0, 4}, {5, 5, 5, 5}, 6, nullptr);
}

void test_sets_validation() {
  char err[256] = "";
  const uint32_t NO = BLS_SET_NO_COMMITTEE;
  const uint32_t sc[3] = {BLS_COMMITTEE_REF(1, 2), NO, BLS_COMMITTEE_REF(0, 0)};
  const uint32_t bo[4] = {0, 2, 2, 3};
  const uint32_t po[4] = {0, 0, 3, 3};
  const uint8_t bits[3] = {1, 2, 3};
  bls_committee_sets cs = {sc, bo, bits};
  CHECK(committee_check_sets(&cs, 3, po, err, sizeof(err)) == 0);
  CHECK(committee_check_sets(&cs, 3, nullptr, err, sizeof(err)) == 0);
  CHECK(committee_check_sets(nullptr, 3, po, err, sizeof(err)) == -2);
  CHECK(committee_check_sets(nullptr, 0, po, err, sizeof(err)) == -2);
  const uint32_t bo_back[4] = {0, 2, 1, 3};
  cs.set_bits_off = bo_back;
  CHECK(committee_check_sets(&cs, 3, po, err, sizeof(err)) == -2 && strstr(err, "not monotone at set 1"));
  const uint32_t bo_no[4] = {0, 2, 3, 3};  // the NO_COMMITTEE set carries a byte
  cs.set_bits_off = bo_no;
  CHECK(committee_check_sets(&cs, 3, po, err, sizeof(err)) == -2 && strstr(err, "set 1 names no committee"));
  const uint32_t bo_first[4] = {1, 2, 2, 3};
  cs.set_bits_off = bo_first;
  CHECK(committee_check_sets(&cs, 3, po, err, sizeof(err)) == -2 && strstr(err, "set_bits_off[0]"));
  cs.set_bits_off = bo;
  const uint32_t po_list[4] = {0, 1, 3, 3};  // a committee set with an index list of its own
  CHECK(committee_check_sets(&cs, 3, po_list, err, sizeof(err)) == -2 && strstr(err, "set 0 names a committee"));
  cs.bits = nullptr;
  CHECK(committee_check_sets(&cs, 3, po, err, sizeof(err)) == -2 && strstr(err, "bits missing"));
  CHECK(BLS_COMMITTEE_REF(7, 0xFFFFFF) == 0x07FFFFFFu);
  CHECK(committee_ref_group(BLS_COMMITTEE_REF(5, 77)) == 5 && committee_ref_index(BLS_COMMITTEE_REF(5, 77)) == 77);
  CHECK(committee_ref_group(NO) == 255);  // never a group
}

void test_slots() {
  const long allocs0 = g_allocs, frees0 = g_frees;
  const std::vector<uint32_t> off_a = {0, 3, 4, 8}, mem_a = {0, 1, 2, 9, 4, 4, 5, 6};
  const std::vector<uint32_t> off_b = {0, 2}, mem_b = {7, 7};
  {
    CommitteeSlots slots(&MEM, TOTAL_BYTES);
    const char* what = nullptr;
    for (uint32_t g = 0; g < BLS_COMMITTEE_GROUPS; ++g) {
      const bls_committee_info i = slots.info(g);
      CHECK(i.n_committees == 0 && i.n_members == 0 && i.device_bytes == 0);
    }
    CHECK(slots.set(2, 3, off_a.data(), mem_a.data(), upload, totals, &what) == 0);
    CHECK(live_blocks() == 1);
    bls_committee_info i = slots.info(2);
    const CommitteeLayout la = committee_layout(3, 8, TOTAL_BYTES);
    CHECK(i.n_committees == 3 && i.n_members == 8 && i.device_bytes == la.bytes);
    CHECK(la.members_at % 256 == 0 && la.totals_at % 256 == 0 && la.members_at >= 16 && la.bytes == la.totals_at + 24);
    CHECK(live_bytes() == la.bytes && slots.device_bytes() == la.bytes);
    CommitteeGroupDev v[BLS_COMMITTEE_GROUPS];
    slots.views(v);
    CHECK(v[2].n == 3 && v[2].offsets && v[0].offsets == nullptr && v[0].n == 0);
    CHECK(memcmp(v[2].offsets, off_a.data(), 16) == 0 && memcmp(v[2].members, mem_a.data(), 32) == 0);
    CHECK(((const Z*)v[2].totals)[1] == key_at(9));
    CHECK(((const Z*)v[2].totals)[2] == 2 * key_at(4) + key_at(5) + key_at(6));  // with multiplicity
    // a second group beside it, then a replacement of the first: one free, one allocation
    CHECK(slots.set(0, 1, off_b.data(), mem_b.data(), upload, totals, &what) == 0);
    CHECK(live_blocks() == 2);
    CHECK(slots.set(2, 1, off_b.data(), mem_b.data(), upload, totals, &what) == 0);
    CHECK(live_blocks() == 2 && g_frees - frees0 == 1);
    i = slots.info(2);
    CHECK(i.n_committees == 1 && i.n_members == 2);
    slots.views(v);
    CHECK(((const Z*)v[2].totals)[0] == 2 * key_at(7));
    CHECK(slots.device_bytes() == live_bytes());
    // failures leave the slot as it was and leak nothing
    const uint8_t* before = (const uint8_t*)v[2].offsets;
    g_fail_next = true;
    CHECK(slots.set(2, 3, off_a.data(), mem_a.data(), upload, totals, &what) == -1 && strstr(what, "allocation"));
    g_fail_totals = true;
    CHECK(slots.set(2, 3, off_a.data(), mem_a.data(), upload, totals, &what) == -1 && strstr(what, "totals"));
    g_fail_totals = false;
    const auto no_upload = [](void*, const void*, size_t) { return false; };
    CHECK(slots.set(2, 3, off_a.data(), mem_a.data(), no_upload, totals, &what) == -1 && strstr(what, "copy"));
    slots.views(v);
    CHECK((const uint8_t*)v[2].offsets == before && slots.info(2).n_committees == 1 && live_blocks() == 2);
    // drop: once frees, twice is a no-op
    CHECK(slots.set(2, 0, nullptr, nullptr, upload, totals, &what) == 0);
    CHECK(live_blocks() == 1 && slots.info(2).device_bytes == 0);
    CHECK(slots.set(2, 0, nullptr, nullptr, upload, totals, &what) == 0);
    CHECK(live_blocks() == 1);
    slots.views(v);
    CHECK(v[2].offsets == nullptr && v[2].n == 0);
    CHECK(slots.set(5, 3, off_a.data(), mem_a.data(), upload, totals, &what) == 0);
    CHECK(live_blocks() == 2);
  }  // close: the destructor frees groups 0 and 5
  CHECK(live_blocks() == 0);
  CHECK(g_allocs - allocs0 == g_frees - frees0);
  CHECK(g_allocs - allocs0 == 6);  // groups 2, 0, 2 again, 5, and the two freed at once after failing totals / copy
}

void test_rules() {
  // the tie: n = 8, c = 4 costs 4 directly and 8 - 4 + 1 = 5 by complement; c = 5: 5 against 4
  CHECK(!committee_use_complement(8, 4));
  CHECK(committee_use_complement(8, 5));
  CHECK(!committee_use_complement(1, 0) && !committee_use_complement(1, 1));
  for (uint32_t n : {1u, 2u, 7u, 8u, 9u, 64u, 65u, 512u, BLS_COMMITTEE_MAX_MEMBERS}) {
    CHECK(!committee_use_complement(n, 0));
    CHECK(committee_use_complement(n, n) == (n > 1));  // the total alone: one addition of -0
    for (uint32_t c = 0; c <= n && c <= 600; ++c) {
      const bool comp = committee_use_complement(n, c);
      CHECK(comp == ((long long)n - c + 1 < (long long)c));
      // strictly fewer additions, never a tie broken towards the complement
      if (comp) CHECK(n - c + 1 < c);
      else CHECK(n - c + 1 >= c);
    }
  }
  CHECK(committee_use_complement(0xFFFFFFFFu, 0xFFFFFFFFu));  // no wrap in n - c + 1
  CHECK(!committee_use_complement(0xFFFFFFFFu, 0x7FFFFFFFu));
  CHECK(committee_weight(512, 507) == 6 && committee_weight(512, 5) == 6 && committee_weight(8, 4) == 5);
  CHECK(committee_weight(1, 1) == 1 && committee_weight(1, 0) == 1);

  // length and padding
  for (uint32_t n : {1u, 7u, 8u, 9u, 64u, 65u}) {
    const uint32_t nb = committee_bits_bytes(n);
    CHECK(nb == (n + 7) / 8);
    std::vector<uint8_t> bits(nb + 1, 0);
    CHECK(committee_check_bits(bits.data(), nb, n) == BLS_CODE_OK);
    CHECK(committee_check_bits(bits.data(), nb + 1, n) == BLS_CODE_BAD_ENCODING);
    CHECK(committee_check_bits(bits.data(), nb - 1, n) == BLS_CODE_BAD_ENCODING);
    CHECK(committee_check_bits(bits.data(), 0, n) == BLS_CODE_BAD_ENCODING);
    // every bit below n is a member's; every bit of the last byte at or past n is padding
    for (uint32_t j = 0; j < 8 * nb; ++j) {
      std::fill(bits.begin(), bits.end(), 0);
      bits[j >> 3] = (uint8_t)(1u << (j & 7));
      CHECK(committee_check_bits(bits.data(), nb, n) == (j < n ? BLS_CODE_OK : BLS_CODE_BAD_ENCODING));
      if (j < n) {
        CHECK(committee_bit(bits.data(), j) && committee_popcount(bits.data(), n) == 1);
        CHECK(committee_selects(bits.data(), j, false) && !committee_selects(bits.data(), j, true));
      }
    }
    std::fill(bits.begin(), bits.end(), 0xFF);
    CHECK(committee_check_bits(bits.data(), nb, n) == ((n & 7) ? BLS_CODE_BAD_ENCODING : BLS_CODE_OK));
    CHECK(committee_padding_mask(n) == ((n & 7) ? (uint32_t)(0xFF << (n & 7)) & 0xFF : 0u));
  }
}

// the single-lane statement over integers: both branches equal the plain sum over set bits
void test_selection() {
  uint32_t seed = 12345;
  const auto rnd = [&]() { return seed = seed * 1664525u + 1013904223u; };
  const auto at = [](uint32_t m) { return key_at(m); };
  const auto add = [](Z a, Z b) { return a + b; };
  const auto neg = [](Z a) { return (Z)0 - a; };
  int direct = 0, complement = 0;
  for (uint32_t n : {1u, 2u, 7u, 8u, 9u, 63u, 64u, 65u, 129u, 512u}) {
    std::vector<uint32_t> mem(n);
    for (uint32_t j = 0; j < n; ++j) mem[j] = rnd() % 97;  // duplicates on purpose
    Z total = 0;
    for (uint32_t j = 0; j < n; ++j) total += key_at(mem[j]);
    std::vector<std::vector<uint8_t>> fields;
    const uint32_t nb = committee_bits_bytes(n);
    const auto field_of = [&](auto pred) {
      std::vector<uint8_t> f(nb, 0);
      for (uint32_t j = 0; j < n; ++j)
        if (pred(j)) f[j >> 3] |= (uint8_t)(1u << (j & 7));
      return f;
    };
    fields.push_back(field_of([](uint32_t) { return true; }));
    fields.push_back(field_of([](uint32_t) { return false; }));
    fields.push_back(field_of([](uint32_t j) { return j == 0; }));
    fields.push_back(field_of([&](uint32_t j) { return j == n - 1; }));
    fields.push_back(field_of([](uint32_t j) { return j != 0; }));
    fields.push_back(field_of([&](uint32_t j) { return j != n - 1; }));
    fields.push_back(field_of([](uint32_t j) { return (j & 1) == 0; }));
    for (int d = -1; d <= 1; ++d)
      fields.push_back(field_of([&](uint32_t j) { return (int)j < (int)(n / 2) + d; }));
    for (int k = 0; k < 8; ++k) {
      const uint32_t density = rnd() % 101;
      fields.push_back(field_of([&](uint32_t) { return rnd() % 100 < density; }));
    }
    for (const auto& f : fields) {
      CHECK(committee_check_bits(f.data(), nb, n) == BLS_CODE_OK);
      Z want = 0;
      uint32_t c = 0;
      for (uint32_t j = 0; j < n; ++j)
        if (committee_bit(f.data(), j)) want += key_at(mem[j]), ++c;
      CHECK(c == committee_popcount(f.data(), n));
      const Z got = committee_select_sum<Z>(mem.data(), n, f.data(), total, (Z)0, true, at, add, neg);
      const Z plain = committee_select_sum<Z>(mem.data(), n, f.data(), total, (Z)0, false, at, add, neg);
      CHECK(got == want);
      CHECK(plain == want);
      // a wrong total must show exactly when the complement is taken
      const Z off = committee_select_sum<Z>(mem.data(), n, f.data(), total + 1, (Z)0, true, at, add, neg);
      CHECK((off != want) == committee_use_complement(n, c));
      (committee_use_complement(n, c) ? complement : direct)++;
    }
  }
  CHECK(direct > 20 && complement > 20);
}

}  // namespace

int main() {
  test_validation();
  test_sets_validation();
  test_slots();
  test_rules();
  test_selection();
  if (g_failed) {
    fprintf(stderr, "committee_host: %d checks failed\n", g_failed);
    return 1;
  }
  printf("ok %ld\n", g_checks);
  return 0;
}
