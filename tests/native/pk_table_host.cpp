// bls/pk_table.hpp on the CPU: the shared key table's bookkeeping (generations, snapshots,
// appends) over a host allocator that poisons what it frees.  Reader threads take snapshots
// and check that [0, n) of the table and [0, comb_n) of the rows hold the expected pattern
// while a loader appends through several growths, one failing batch among them; a second
// table loses its rows to a failed allocation and a third to a failed build.  Stand-alone:
// prints "ok <checks>" and exits 0, or says what failed and exits 1.  Built plain and with
// -fsanitize=thread / -fsanitize=address by tests/test_pk_table_cpu.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

#include "bls/pk_table.hpp"

using namespace bls;

namespace {

constexpr size_t ENTRY = 100, ROW = 144;  // (the device's rows are 1,440 B: the bookkeeping only scales them)
constexpr uint8_t POISON = 0xDD;

std::atomic<long> g_checks{0};
std::atomic<int> g_failed{0};
#define CHECK(cond)                                                       \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) {                                                        \
      if (!g_failed.exchange(1)) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                     \
  } while (0)

// ---- the allocator: every buffer is poisoned when freed and kept until the program ends, so
// a reader of a freed generation sees POISON (and, under a sanitizer, races with the memset)
struct Block {
  uint8_t* p;
  size_t bytes;
  bool live;
};
std::mutex g_heap_mu;
std::vector<Block> g_heap;
std::atomic<long> g_allocs{0}, g_frees{0};
std::atomic<size_t> g_fail_bytes{0};  // the next allocation of exactly this size fails (once)

void* h_alloc(size_t bytes) {
  size_t want = bytes;
  if (g_fail_bytes.compare_exchange_strong(want, 0)) return nullptr;
  uint8_t* p = (uint8_t*)malloc(bytes);
  memset(p, 0xA5, bytes);
  std::lock_guard<std::mutex> g(g_heap_mu);
  g_heap.push_back(Block{p, bytes, true});
  ++g_allocs;
  return p;
}
void h_free(void* p) {
  size_t bytes = 0;
  {
    std::lock_guard<std::mutex> g(g_heap_mu);
    for (Block& b : g_heap)
      if (b.p == p) {
        CHECK(b.live);  // no double free
        b.live = false;
        bytes = b.bytes;
      }
  }
  CHECK(bytes != 0);
  memset(p, POISON, bytes);
  ++g_frees;
}
bool h_copy(void* dst, const void* src, size_t bytes, void*) {
  memcpy(dst, src, bytes);
  return true;
}
bool h_sync(void*) { return true; }
const PkMem MEM = {h_alloc, h_free, h_copy, h_sync};

long live_blocks() {
  std::lock_guard<std::mutex> g(g_heap_mu);
  long n = 0;
  for (const Block& b : g_heap) n += b.live;
  return n;
}

uint8_t key_byte(uint32_t i, size_t j) { return (uint8_t)(i * 131u + j * 7u + 1u); }
uint8_t row_byte(uint32_t i, size_t j) { return (uint8_t)(i * 17u + j * 3u + 5u); }

void write_keys(uint8_t* dst, uint32_t first, uint32_t m) {
  for (uint32_t k = 0; k < m; ++k)
    for (size_t j = 0; j < ENTRY; ++j) dst[ENTRY * k + j] = key_byte(first + k, j);
}
bool write_rows(const PkGen& g, uint32_t from, uint32_t to) {
  for (uint32_t i = from; i < to; ++i) {
    for (size_t j = 0; j < ROW; ++j) g.comb_p()[ROW * i + j] = row_byte(i, j);
    g.comb_ok_p()[i] = 1;
  }
  return true;
}

// what a verify call does with its snapshot: reads [0, n) and the rows [0, comb_n), nothing else
void check_snapshot(const PkSnapshot& s) {
  const PkGen& g = *s.gen;
  CHECK(s.n <= g.cap);
  CHECK(s.comb_n <= g.comb_cap && g.comb_cap <= g.cap && s.comb_n <= s.n);
  CHECK((g.comb_p() != nullptr) == (g.comb_ok_p() != nullptr));
  if (!g.comb_p()) CHECK(s.comb_n == 0);
  bool keys = true, rows = true;
  for (uint32_t i = 0; i < s.n && keys; ++i)
    for (size_t j = 0; j < ENTRY; ++j) keys = keys && g.table_p()[ENTRY * i + j] == key_byte(i, j);
  for (uint32_t i = 0; i < s.comb_n && rows; ++i) {
    rows = g.comb_ok_p()[i] == 1;
    for (size_t j = 0; j < ROW; ++j) rows = rows && g.comb_p()[ROW * i + j] == row_byte(i, j);
  }
  CHECK(keys);
  CHECK(rows);
}

struct Loader {
  PkTable& t;
  uint32_t comb_max;
  bool build_fails = false;
  // m keys; bad: one of them does not decode (its slots are scribbled on, nothing published)
  int64_t load(uint32_t m, bool bad = false) {
    const uint32_t n0 = t.size();
    const char* what = nullptr;
    return t.append(
        m, comb_max, nullptr,
        [&](uint8_t* dst) {
          if (bad) {
            memset(dst, 0xEE, ENTRY * m);
            return 1;
          }
          write_keys(dst, n0, m);
          return 0;
        },
        [&](const PkGen& g, uint32_t from, uint32_t to) { return !build_fails && write_rows(g, from, to); }, &what);
  }
};

// readers against one loader: growths, a failing batch, a rows cap reached on the way
void readers_and_loader() {
  const uint32_t COMB_MAX = 3000;
  auto table = std::make_shared<PkTable>(&MEM, 0, ENTRY, ROW, false);
  table->attach();
  std::atomic<bool> done{false};
  std::atomic<long> snaps{0}, gens_seen{0};
  std::vector<std::thread> readers;
  for (int r = 0; r < 4; ++r)
    readers.emplace_back([&] {
      uint32_t last_n = 0;
      const PkGen* last_gen = nullptr;
      while (!done.load()) {
        PkSnapshot s = table->snapshot();
        CHECK(s.n >= last_n);  // the table only grows
        last_n = s.n;
        if (s.gen.get() != last_gen) ++gens_seen;
        last_gen = s.gen.get();
        check_snapshot(s);  // (the snapshot is held over the whole check, as over a call)
        ++snaps;
      }
    });
  Loader ld{*table, COMB_MAX};
  uint32_t n = 0, caps = 0, last_cap = 0;
  const uint32_t batches[] = {3, 70, 1100, 1, 0, 900, 2500, 1, 4000};
  int k = 0;
  for (uint32_t m : batches) {
    if (k++ == 5) {  // a batch with an undecodable key, large enough to grow the table first
      const int64_t r = ld.load(2000, true);
      CHECK(r == (int64_t)n);
      CHECK(table->size() == n);
    }
    const int64_t r = ld.load(m);
    n += m;
    CHECK(r == (int64_t)n);
    const PkInfo i = table->info();
    CHECK(i.n_keys == n && i.capacity >= n && i.n_contexts == 1 && i.table_id == table->id());
    CHECK(i.comb_keys == (n < COMB_MAX ? n : COMB_MAX));
    const uint32_t comb_cap = i.capacity < COMB_MAX ? i.capacity : COMB_MAX;
    CHECK(i.device_bytes == (uint64_t)i.capacity * ENTRY + (uint64_t)comb_cap * (ROW + 1));
    if (i.capacity != last_cap) ++caps;
    last_cap = i.capacity;
    if (k == 1) CHECK(i.capacity == 3 + 1 + 1024);  // the first capacity (3 keys): 1,028
    std::this_thread::yield();
  }
  CHECK(caps >= 4);  // several growths (the failing batch's among them)
  while (snaps.load() < 8) std::this_thread::yield();
  done = true;
  for (auto& t : readers) t.join();
  check_snapshot(table->snapshot());
  // a snapshot outlives the table's own reference to its generation, and the table itself
  PkSnapshot old = table->snapshot();
  ld.load(9000);
  check_snapshot(old);
  CHECK(old.gen != table->snapshot().gen);
  table->detach();
  table.reset();
  check_snapshot(old);
  const long before = live_blocks();
  CHECK(before == 3);  // the snapshot's table, rows and comb_ok
  old = PkSnapshot();
  CHECK(live_blocks() == 0);
  CHECK(gens_seen.load() >= 4);
}

// the rows' allocation fails at a growth: the table goes on without rows, an earlier
// snapshot keeps its own
void comb_allocation_fails() {
  PkTable t(&MEM, 0, ENTRY, ROW, false);
  Loader ld{t, 1u << 20};
  CHECK(ld.load(10) == 10);
  const PkSnapshot with_rows = t.snapshot();
  CHECK(with_rows.comb_n == 10 && with_rows.gen->comb_p());
  const uint32_t cap = (2000 + 10) + (2000 + 10) / 2 + 1024;
  g_fail_bytes = ROW * (size_t)cap;
  CHECK(ld.load(2000) == 2010);
  CHECK(g_fail_bytes.load() == 0);  // (it was this allocation that failed)
  const PkSnapshot bare = t.snapshot();
  CHECK(bare.n == 2010 && bare.comb_n == 0 && !bare.gen->comb_p() && !bare.gen->comb_ok_p());
  check_snapshot(bare);
  check_snapshot(with_rows);
  CHECK(ld.load(5000) == 7010);  // and never tries again
  CHECK(t.info().comb_keys == 0 && t.info().device_bytes == (uint64_t)t.info().capacity * ENTRY);
  check_snapshot(t.snapshot());
  // the table's own allocation fails: the load fails, the table is as it was
  const uint32_t cap2 = (7010 + 60000) + (7010 + 60000) / 2 + 1024;
  g_fail_bytes = ENTRY * (size_t)cap2;
  const char* what = nullptr;
  CHECK(t.append(60000, 0, nullptr, [](uint8_t*) { return 0; }, [](const PkGen&, uint32_t, uint32_t) { return true; },
                 &what) == -1);
  CHECK(what != nullptr && t.size() == 7010);
  check_snapshot(t.snapshot());
}

// the rows' build fails: a generation without rows over the same table buffer is published
// with the new keys; an earlier snapshot keeps its rows
void comb_build_fails() {
  PkTable t(&MEM, 0, ENTRY, ROW, false);
  Loader ld{t, 1u << 20};
  CHECK(ld.load(20) == 20);
  const PkSnapshot with_rows = t.snapshot();
  ld.build_fails = true;
  CHECK(ld.load(30) == 50);
  const PkSnapshot bare = t.snapshot();
  CHECK(bare.n == 50 && bare.comb_n == 0 && !bare.gen->comb_p());
  CHECK(bare.gen->table_p() == with_rows.gen->table_p());  // no copy of the keys
  CHECK(with_rows.comb_n == 20);
  check_snapshot(with_rows);
  check_snapshot(bare);
  ld.build_fails = false;
  CHECK(ld.load(5) == 55 && t.info().comb_keys == 0);
}

// no rows at all ($BLS_PK_COMB=0), distinct ids, the context count
void plain_tables() {
  PkTable a(&MEM, 0, ENTRY, ROW, true), b(&MEM, 1, ENTRY, ROW, true);
  CHECK(a.id() != 0 && b.id() != 0 && a.id() != b.id());
  CHECK(a.device() == 0 && b.device() == 1);
  a.attach();
  a.attach();
  CHECK(a.info().n_contexts == 2);
  a.detach();
  CHECK(a.info().n_contexts == 1);
  Loader ld{a, 1u << 20};
  CHECK(ld.load(0) == 0);
  CHECK(ld.load(1500) == 1500);
  const PkInfo i = a.info();
  CHECK(i.comb_keys == 0 && i.device_bytes == (uint64_t)i.capacity * ENTRY);
  check_snapshot(a.snapshot());
  void* rows = MEM.alloc(64);
  b.set_g1_comb(rows);  // owned by the table from here
  CHECK(b.g1_comb() == rows);
}

}  // namespace

int main() {
  readers_and_loader();
  CHECK(live_blocks() == 0);
  comb_allocation_fails();
  CHECK(live_blocks() == 0);
  comb_build_fails();
  CHECK(live_blocks() == 0);
  plain_tables();
  CHECK(live_blocks() == 0);
  CHECK(g_allocs.load() == g_frees.load());
  for (Block& b : g_heap) {
    bool poisoned = true;
    for (size_t j = 0; j < b.bytes; ++j) poisoned = poisoned && b.p[j] == POISON;
    CHECK(poisoned);  // nothing wrote to a buffer after its free
    free(b.p);
  }
  if (g_failed.load()) return 1;
  printf("ok %ld\n", g_checks.load());
  return 0;
}
