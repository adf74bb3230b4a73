// The device public-key table as an object of its own: one per device, shared by the
// contexts that bls_gpu_share_pubkeys joined (a context that never shares owns a private
// one).  Host-side bookkeeping only -- the device allocation, copy and free sit behind
// PkMem, so this file also compiles for the CPU (tests/native/pk_table_host.cpp).
//
//   generation  one set of buffers: the table, the comb rows, comb_ok, and their
//               capacities.  Reference-counted; the buffers are freed with the last
//               reference.  (Each buffer carries its own count, so a generation that only
//               drops the rows, or whose rows are at their cap, shares the rest with its
//               predecessor instead of copying it.)
//   snapshot    what a call hands to its kernels: a generation reference, n and comb_n,
//               taken once under the short mutex and dropped after the call's last stream
//               synchronisation.  Kernels never read slots at or above their snapshot's n.
//   append      under the loader mutex, on the calling context's stream.  Keys that fit
//               are decoded into slots [n, n + m) of the current generation and their rows
//               built, each followed by a stream synchronisation; only then are n and
//               comb_n published under the short mutex, so readers are never blocked and
//               kernels that other contexts launch afterwards see finished memory.  Keys
//               that do not fit go to a new generation: [0, n) and the built rows copied
//               device-to-device, synchronised, then the generation swapped under the short
//               mutex; the old one is freed when its last reader drops it, outside both
//               mutexes (a device free may wait for the device).
// Lock order: a context's mutex, then the loader mutex, then the short mutex.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

namespace bls {

// device memory as the table sees it (streams are opaque)
struct PkMem {
  void* (*alloc)(size_t bytes);  // nullptr: no memory
  void (*free)(void* p);
  bool (*copy)(void* dst, const void* src, size_t bytes, void* stream);  // device to device, on the stream
  bool (*sync)(void* stream);
};

struct PkBuf {
  const PkMem* mem;
  uint8_t* p;
  size_t bytes;
  PkBuf(const PkMem* m, uint8_t* ptr, size_t b) : mem(m), p(ptr), bytes(b) {}
  PkBuf(const PkBuf&) = delete;
  PkBuf& operator=(const PkBuf&) = delete;
  ~PkBuf() {
    if (p) mem->free(p);
  }
  static std::shared_ptr<PkBuf> make(const PkMem* m, size_t bytes) {
    void* p = m->alloc(bytes ? bytes : 1);
    return p ? std::make_shared<PkBuf>(m, (uint8_t*)p, bytes) : nullptr;
  }
};

struct PkGen {
  std::shared_ptr<PkBuf> table, comb, comb_ok;  // comb, comb_ok: both or neither
  uint32_t cap = 0, comb_cap = 0;               // keys; comb_cap <= cap
  uint8_t* table_p() const { return table ? table->p : nullptr; }
  uint8_t* comb_p() const { return comb ? comb->p : nullptr; }
  uint8_t* comb_ok_p() const { return comb_ok ? comb_ok->p : nullptr; }
  uint64_t bytes() const {
    return (uint64_t)(table ? table->bytes : 0) + (comb ? comb->bytes : 0) + (comb_ok ? comb_ok->bytes : 0);
  }
};

struct PkSnapshot {
  std::shared_ptr<const PkGen> gen;
  uint32_t n = 0, comb_n = 0;
};

struct PkInfo {
  uint64_t table_id;
  uint32_t n_keys, capacity, comb_keys, n_contexts;
  uint64_t device_bytes;
};

class PkTable {
 public:
  // entry_bytes, row_bytes: one key's table entry and its comb rows; comb_off: no rows
  PkTable(const PkMem* mem, int device, size_t entry_bytes, size_t row_bytes, bool comb_off)
      : mem_(mem), device_(device), entry_(entry_bytes), row_(row_bytes), id_(next_id()),
        gen_(std::make_shared<PkGen>()), comb_off_(comb_off) {}
  PkTable(const PkTable&) = delete;
  PkTable& operator=(const PkTable&) = delete;
  ~PkTable() {
    if (g1_comb_) mem_->free(g1_comb_);
  }

  int device() const { return device_; }
  uint64_t id() const { return id_; }

  // the generator's rows: set once, before the table has a second user; owned from then on
  void set_g1_comb(void* rows) { g1_comb_ = rows; }
  const void* g1_comb() const { return g1_comb_; }

  PkSnapshot snapshot() const {
    std::lock_guard<std::mutex> g(mu_);
    return PkSnapshot{gen_, n_, comb_n_};
  }
  uint32_t size() const {
    std::lock_guard<std::mutex> g(mu_);
    return n_;
  }
  PkInfo info() const {
    std::lock_guard<std::mutex> g(mu_);
    return PkInfo{id_, n_, gen_->cap, comb_n_, n_ctx_, gen_->bytes()};
  }
  void attach() {
    std::lock_guard<std::mutex> g(mu_);
    ++n_ctx_;
  }
  void detach() {
    std::lock_guard<std::mutex> g(mu_);
    --n_ctx_;
  }

  // Append m keys.  decode(dst) writes them to dst (slots [n, n + m) of the table) on the
  // stream and waits for it: 0 all decoded, 1 some key did not (nothing is published), < 0
  // a device error.  build(gen, from, to) writes the rows and comb_ok of keys [from, to) of
  // gen on the stream and waits: false drops the comb for the table (a generation without
  // rows is published; a reader's snapshot keeps what it had).  comb_max_keys: the rows'
  // cap for the table.  Returns the table's size afterwards, or -1 with *what naming the
  // step (the table is then as it was).
  template <class Decode, class Build>
  int64_t append(uint32_t m, uint32_t comb_max_keys, void* stream, Decode&& decode, Build&& build,
                 const char** what) {
    // generations this load replaced: released after both mutexes (declared first)
    std::vector<std::shared_ptr<const PkGen>> retired;
    std::lock_guard<std::mutex> loader(load_mu_);
    // only a loader writes gen_, n_, comb_n_ and comb_off_, so this one reads them unlocked
    const uint32_t n0 = n_;
    if ((uint64_t)n0 + m > 0xFFFFFFFFull) return fail(what, "table index overflow");
    if (n0 + m > gen_->cap) {
      const uint64_t cap64 = (uint64_t)(n0 + m) + (n0 + m) / 2 + 1024;
      const uint32_t cap = cap64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap64;
      auto g = std::make_shared<PkGen>();
      g->cap = cap;
      if (!(g->table = PkBuf::make(mem_, entry_ * (size_t)cap))) return fail(what, "table allocation");
      bool copied = false;
      if (n0) {
        if (!mem_->copy(g->table->p, gen_->table_p(), entry_ * (size_t)n0, stream)) return fail(what, "table copy");
        copied = true;
      }
      bool drop = false;
      if (!comb_off_) {
        const uint32_t want = cap < comb_max_keys ? cap : comb_max_keys;
        if (want <= gen_->comb_cap) {  // the rows are at their cap: the same buffers serve
          g->comb = gen_->comb;
          g->comb_ok = gen_->comb_ok;
          g->comb_cap = gen_->comb_cap;
        } else {
          g->comb = PkBuf::make(mem_, row_ * (size_t)want);
          g->comb_ok = g->comb ? PkBuf::make(mem_, want) : nullptr;
          bool good = g->comb && g->comb_ok;
          if (good && comb_n_) {
            good = mem_->copy(g->comb->p, gen_->comb_p(), row_ * (size_t)comb_n_, stream) &&
                   mem_->copy(g->comb_ok->p, gen_->comb_ok_p(), comb_n_, stream);
            copied = true;
          }
          g->comb_cap = want;
          if (!good) drop = true;
        }
      }
      if (copied && !mem_->sync(stream)) return fail(what, "table copy");
      if (drop) {
        g->comb = g->comb_ok = nullptr;
        g->comb_cap = 0;
      }
      std::lock_guard<std::mutex> lk(mu_);
      retired.push_back(std::move(gen_));
      gen_ = std::move(g);
      if (drop) {
        comb_off_ = true;
        comb_n_ = 0;
      }
    }
    if (m == 0) return n0;
    const int rc = decode(gen_->table_p() + entry_ * (size_t)n0);
    if (rc < 0) return fail(what, "key decode");
    if (rc > 0) return n0;  // all or nothing, for every sharer at once
    uint32_t comb_n = comb_n_;
    std::shared_ptr<PkGen> bare;
    if (!comb_off_ && gen_->comb) {
      const uint32_t end = n0 + m < gen_->comb_cap ? n0 + m : gen_->comb_cap;
      if (end > comb_n) {
        if (build(*gen_, comb_n, end)) {
          comb_n = end;
        } else {
          bare = std::make_shared<PkGen>();
          bare->table = gen_->table;
          bare->cap = gen_->cap;
          comb_n = 0;
        }
      }
    }
    std::lock_guard<std::mutex> lk(mu_);
    if (bare) {
      retired.push_back(std::move(gen_));
      gen_ = std::move(bare);
      comb_off_ = true;
    }
    n_ = n0 + m;
    comb_n_ = comb_n;
    return n_;
  }

 private:
  static uint64_t next_id() {
    static std::atomic<uint64_t> last{0};
    return ++last;
  }
  static int64_t fail(const char** what, const char* msg) {
    if (what) *what = msg;
    return -1;
  }

  const PkMem* const mem_;
  const int device_;
  const size_t entry_, row_;
  const uint64_t id_;
  void* g1_comb_ = nullptr;
  mutable std::mutex mu_;  // the short mutex: gen_, n_, comb_n_, n_ctx_ as readers see them
  std::mutex load_mu_;     // one load at a time
  std::shared_ptr<PkGen> gen_;
  uint32_t n_ = 0, comb_n_ = 0, n_ctx_ = 0;
  bool comb_off_;
};

}  // namespace bls
