// MI355X (gfx950) BLS12-381 signature-set verifier: host orchestration and the
// C-ABI declared in include/lodestar_bls.h.  Kernels: lodestar_amd/csrc/kernels/*.hip;
// single-lane bodies in bls/pipeline.hpp, host-side plans in bls/plan.hpp (both shared with
// the CPU test harness); cooperative programs from tools/gen_coop.py.
//
// Every verify entry point (bls_gpu_verify, _verify_many, _verify_same_message, _partial,
// _verify_deposits) is one VerifyPass (below): plan_pass (bls/plan.hpp) fixes its shape and plans from the
// process's knobs (bls/knobs.hpp: the BLS_* variables and the decisions taken from them),
// then verify_body calls its stages in order.  The inputs sit in pinned mapped staging memory (no H2D copy), all
// kernels run on the context's stream, and the host waits after the first pass and after
// each fallback round.
//   k_pk, k_pre   pubkey decode / table aggregation; SSWU points of H(m), signature decode
//                 (a deposit call: k_deposit in k_pk's place -- KeyValidate of the
//                 compressed keys and the signing roots, made on the device)
//   first pass, one of two shapes (use_sigagg):
//     per set     k_pset (k_psetn: up to 3 sets per wavefront): H(m), G2 subgroup test,
//                 r pk, r g1, f_i = ML(r pk, H) ML(-r g1, sig), one wavefront per set
//     aggregated  k_chain (per-set chains, one lane each), then the signature sums into
//                 virtual sets -- k_gsum levels + k_vset per chunk, or ONE sum for the pass
//                 (use_total) by k_gsum or the Pippenger k_msm, or k_smsum per same-message
//                 job -- then the Miller-loop units' sums r_i pk_i per shared root (k_gsum1 +
//                 k_uset), then every Miller loop in one launch (k_mln)
//   k_status      per-request error precedence
//   merged check  FE(prod of every f) == 1 by one k_fprod tree, when every request is
//                 batchable and there are >= 2 chunks
// and, as far as the pass has to go down the fallback ladder:
//   flagged redo  k_exact (complete formulas) for the rare sets the cooperative kernels
//                 flagged, then k_status and the merged check again
//   chunk checks  no merged check, or it failed: (the chunks' own sums and Miller loops,
//                 when the first pass summed once,) FE per chunk by k_chunk_coop / _simt
//   individual    the non-batchable and the failed chunks' requests: their own Miller
//                 loops and signature sums, k_fold, k_indiv_coop / _simt
//   group tests   failed chunks of >= group_test_min requests: k_group_coop over bit groups
//                 instead of one final exponentiation per request (verify_groups)
// A partial call (one shard of a sharded call) stops after the status and returns the
// product of its f.  DESIGN.md section 3 describes each step and the measurements behind
// the thresholds.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <sys/random.h>
#include <time.h>
#include <unistd.h>

#include <dlfcn.h>
#include <stdlib.h>
#include <zlib.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "bls/committee.hpp"
#include "bls/deposit.hpp"
#include "bls/group_decode.hpp"
#include "bls/knobs.hpp"
#include "bls/pk_table.hpp"
#include "bls/plan.hpp"
#include "launchers.hpp"
#include "kernels/curve_op_ids.hpp"
#include "kernels/tower_op_ids.hpp"

using namespace bls;

struct bls_gpu_ctx {
  int device;
  hipStream_t stream;
  hipEvent_t ev0, ev1;
  hipEvent_t ev[9];  // stage boundaries of the last verify call
  // the event the verify path polls instead of spinning in hipStreamSynchronize when
  // the call's pass is large (wait_block, pass_wait)
  hipEvent_t ev_wait;
  bool wait_block;
  char err[512];
  // The device pubkey table (affine, Montgomery), private until bls_gpu_share_pubkeys joins
  // another context's: bls/pk_table.hpp.  A generation holds the table, the fixed-base
  // comb rows of its keys (curve.hpp g1_comb_mul; k_chain role 3), grown and copied with
  // the table -- room for keys [0, comb_cap), comb_cap <= cap ($BLS_PK_COMB_MAX_MB), of
  // which [0, comb_n) are built -- and comb_ok[i] = 1 where key i has rows.  No rows: off
  // ($BLS_PK_COMB=0) or an allocation failed -- every set then takes the GLV chain; a load
  // never fails because of the comb.  The table also owns the generator's rows, made at
  // its creation (k_pre's RG lanes); nullptr: GLV.  Held through a heap pointer as mu is
  // (the struct is zeroed at creation).  An entry point that hands table pointers to a
  // kernel takes one snapshot and uses only that (pk_snapshot).
  std::shared_ptr<PkTable>* pkt;
  // Committee groups (bls/committee.hpp): the slots' bookkeeping on the host and the eight
  // views the kernels read, in device memory (all zero until a group is registered).
  CommitteeSlots* cm;
  CommitteeGroupDev* cm_dev;
  uint32_t debug_flags;  // bls_gpu_set_debug_flags
  // the context's last pass failed its merged check: its next pass keeps the per-set
  // [r] sig chains rather than the Pippenger sum (plan_pass: PassShape::use_msm), so a failure
  // there does not relaunch them (profiles/r05_ab_msm_min.json)
  bool last_merged_failed;
  // the group-test rounds of the last pass (bls_gpu_group_test_counts; verify_groups)
  uint32_t gt_counts[8];
  // grow-only device workspace and pinned staging
  uint32_t* msm_state;  // MSM bucket counters + tickets (MSM_STATE_WORDS), zero between passes
  uint8_t* dev_ws;
  size_t dev_ws_cap;
  uint8_t* host_stage;      // verify inputs, pinned + device-mapped: kernels read them in place
  uint8_t* host_stage_dev;  // device view of host_stage
  size_t host_stage_cap;
  uint8_t* host_res;        // verify results written by kernels (host-mapped, coherent)
  uint8_t* host_res_dev;
  size_t host_res_cap;
  uint32_t* first_bad;      // two device slots for first_bad_pk (k_pk resets the next call's)
  uint32_t first_bad_slot;
  // cooperative programs (coop_tables.bin, tools/gen_coop.py)
  CoopEnv coop;
  void* coop_dev;
  std::vector<std::pair<std::string, CoopProg>>* coop_progs;
  std::vector<uint32_t>* coop_frames;  // frame size (slots) of coop_progs[k], from the table
  // one call at a time per context: every entry point that touches the stream,
  // workspace or table holds this (callers may share a context across threads)
  std::mutex* mu;
  int admitted;  // counted by the scratch admission (bls_scratch_plan): 0 no, 1 normal, 2 high priority
};

#define CTX_LOCK(ctx) std::lock_guard<std::mutex> ctx_guard_(*(ctx)->mu)

static int set_err(bls_gpu_ctx* ctx, const char* what, hipError_t e) {
  if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s: %s", what, hipGetErrorString(e));
  return -1;
}

#define HIPC(ctx, call)                                     \
  do {                                                      \
    hipError_t e_ = (call);                                 \
    if (e_ != hipSuccess) return set_err((ctx), #call, e_); \
  } while (0)

// ---------------------------------------------------------------------------
// workspace helpers
// ---------------------------------------------------------------------------
namespace {

struct Carver {
  uint8_t* base;
  size_t off;
  uint8_t* host = nullptr;  // offsets below `split` map into this (device view of pinned memory)
  size_t split = 0;
  template <class T>
  T* take(size_t count) {
    off = (off + 255) & ~(size_t)255;
    T* p = (T*)(base ? (off < split && host ? host : base) + off : nullptr);
    off += sizeof(T) * (count ? count : 1);
    return p;
  }
  // take, with the element type read off the pointer it fills; chains: c.buf(a, n).buf(b, m)
  template <class T>
  Carver& buf(T*& p, size_t count) {
    p = take<T>(count);
    return *this;
  }
};

int ensure_dev(bls_gpu_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->dev_ws_cap) return 0;
  if (ctx->dev_ws) HIPC(ctx, hipFree(ctx->dev_ws));
  ctx->dev_ws = nullptr;
  size_t cap = bytes + bytes / 4;
  HIPC(ctx, hipMalloc(&ctx->dev_ws, cap));
  ctx->dev_ws_cap = cap;
  return 0;
}

// One single-launch device call: every entry point below that is no verify pass.  carve()
// takes the call's layout once, as a function over a Carver: it runs without a base for the
// size, grows the workspace, and runs again over it for the pointers.  From its construction
// the object owns the tail of the stream: finish() is the call's one hipStreamSynchronize,
// and every other way out (a failed copy or launch, an early return) waits in the destructor,
// its result ignored so that the first error stays in ctx->err.  Nothing queued then outlives
// the caller's buffers, the workspace or what was declared before the object: the host
// vectors a queued copy reads or writes, and the table snapshot the kernels read.  The entry
// point keeps the lock, hipSetDevice and its argument checks.
struct OneShot {
  bls_gpu_ctx* const ctx;
  const hipStream_t s;
  size_t bytes = 0;  // of the layout
  bool done = false;
  explicit OneShot(bls_gpu_ctx* c) : ctx(c), s(c->stream) {}
  OneShot(const OneShot&) = delete;
  ~OneShot() {
    if (!done) (void)hipStreamSynchronize(s);
  }
  template <class Layout>
  int carve(Layout&& layout) {
    Carver size{nullptr, 0};
    layout(size);
    bytes = size.off;
    if (ensure_dev(ctx, bytes)) return -1;
    Carver at{ctx->dev_ws, 0};
    layout(at);
    return 0;
  }
  int finish() {
    HIPC(ctx, hipStreamSynchronize(s));
    done = true;
    return 0;
  }
};

// Pinned, device-mapped, coherent host memory: the kernels of a verify call read its
// inputs from here and write its results here, so a call moves no data with copy or
// fill blits (those queue behind other contexts' and wait for CU slots under load).
int ensure_mapped(bls_gpu_ctx* ctx, size_t bytes, uint8_t** host, uint8_t** dev, size_t* cap_io) {
  if (bytes <= *cap_io) return 0;
  if (*host) HIPC(ctx, hipHostFree(*host));
  *host = *dev = nullptr;
  size_t cap = bytes + bytes / 4 + 4096;
  HIPC(ctx, hipHostMalloc((void**)host, cap, hipHostMallocMapped | hipHostMallocCoherent));
  HIPC(ctx, hipHostGetDevicePointer((void**)dev, *host, 0));
  *cap_io = cap;
  return 0;
}

int ensure_host(bls_gpu_ctx* ctx, size_t bytes) {
  return ensure_mapped(ctx, bytes, &ctx->host_stage, &ctx->host_stage_dev, &ctx->host_stage_cap);
}

// Write a host array into the staging area behind its device-side pointer.
template <class T>
void stage_copy(bls_gpu_ctx* ctx, const T* dev_ptr, const void* src, size_t bytes) {
  if (!src || !bytes) return;
  size_t off = (const uint8_t*)dev_ptr - ctx->host_stage_dev;
  memcpy(ctx->host_stage + off, src, bytes);
}

// host view of a pointer into the result area
template <class T>
T* res_host(bls_gpu_ctx* ctx, T* dev_ptr) {
  return (T*)(ctx->host_res + ((uint8_t*)dev_ptr - ctx->host_res_dev));
}

}  // namespace

extern "C" int bls_gpu_device_count(void);
extern "C" void bls_gpu_close(bls_gpu_ctx* ctx);
static bool pk_comb_on();  // $BLS_PK_COMB (the comb rows of the table's keys, below)
static void pk_table_new(bls_gpu_ctx* ctx);
static void pk_table_release(bls_gpu_ctx* ctx);
static CommitteeSlots* committee_slots_new();

// ---------------------------------------------------------------------------
// cooperative program tables: lodestar_amd/_native/coop_tables.bin next to this
// library (or $BLS_COOP_TABLES), generated by tools/gen_coop.py at build time.
// ---------------------------------------------------------------------------
namespace {

struct CoopHeader {
  char magic[4];
  uint32_t version, n_consts, n_progs, n_steps;
};
struct CoopProgEntry {
  char name[32];
  uint32_t first, n_steps, frame, n_mul;
};

// the gzip'd table (coop_tables.bin.gz, what travels with the tree) next to the
// library; $BLS_COOP_TABLES may name a plain or gzip'd file (gzread reads both)
std::string coop_tables_path() {
  const char* env = getenv("BLS_COOP_TABLES");
  if (env && *env) return env;
  Dl_info info;
  if (dladdr((void*)&bls_gpu_device_count, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    size_t slash = p.rfind('/');
    return (slash == std::string::npos ? std::string(".") : p.substr(0, slash)) + "/coop_tables.bin.gz";
  }
  return "coop_tables.bin.gz";
}

}  // namespace

static int load_coop_tables(bls_gpu_ctx* ctx) {
  std::string path = coop_tables_path();
  gzFile f = gzopen(path.c_str(), "rb");
  if (!f) {
    snprintf(ctx->err, sizeof(ctx->err), "cannot open %s (run the build: tools/gen_coop.py)", path.c_str());
    return -1;
  }
  std::vector<uint8_t> buf;
  for (;;) {
    const size_t at = buf.size();
    buf.resize(at + (4u << 20));
    const int got = gzread(f, buf.data() + at, 4u << 20);
    if (got < 0) {
      gzclose(f);
      snprintf(ctx->err, sizeof(ctx->err), "read error in %s", path.c_str());
      return -1;
    }
    buf.resize(at + (size_t)got);
    if (got == 0) break;
  }
  gzclose(f);
  const long sz = (long)buf.size();
  const size_t got = buf.size();
  CoopHeader h;
  if (got != (size_t)sz || sz < (long)sizeof(h)) {
    snprintf(ctx->err, sizeof(ctx->err), "short read of %s", path.c_str());
    return -1;
  }
  memcpy(&h, buf.data(), sizeof(h));
  size_t consts_off = sizeof(h), progs_off = consts_off + (size_t)h.n_consts * sizeof(Fp);
  size_t steps_off = progs_off + (size_t)h.n_progs * sizeof(CoopProgEntry);
  size_t steps_bytes = (size_t)h.n_steps * COOP_LANES * sizeof(CoopOp);
  // version 4: lane groups (op kinds 3 / 4, group sizes in the step flags) and the
  // per-step term bounds (coop.hpp CoopOp)
  if (memcmp(h.magic, "BLSC", 4) != 0 || h.version != 4 || steps_off + steps_bytes != (size_t)sz) {
    snprintf(ctx->err, sizeof(ctx->err), "%s: bad coop table format", path.c_str());
    return -1;
  }
  static_assert(sizeof(CoopOp) == 80, "CoopOp layout");
  // device copy: [ops | consts | the CoopEnv struct (filled at the end)]
  const auto layout = [&](Carver& c) {
    c.buf(ctx->coop.ops, (size_t)h.n_steps * COOP_LANES).buf(ctx->coop.consts, h.n_consts).buf(ctx->coop.dev, 1);
  };
  Carver size{nullptr, 0};
  layout(size);
  HIPC(ctx, hipMalloc(&ctx->coop_dev, size.off));
  Carver at{(uint8_t*)ctx->coop_dev, 0};
  layout(at);
  HIPC(ctx, hipMemcpy((void*)ctx->coop.ops, buf.data() + steps_off, steps_bytes, hipMemcpyHostToDevice));
  HIPC(ctx, hipMemcpy((void*)ctx->coop.consts, buf.data() + consts_off, (size_t)h.n_consts * sizeof(Fp),
                      hipMemcpyHostToDevice));
  ctx->coop.n_consts = h.n_consts;
  if (h.n_consts > COOP_MAX_CONSTS) {
    snprintf(ctx->err, sizeof(ctx->err), "%s: %u constants > %d", path.c_str(), h.n_consts, COOP_MAX_CONSTS);
    return -1;
  }
  struct {
    const char* name;
    CoopProg* dst;
  } want[] = {{"fin_fmul", &ctx->coop.fin_fmul},         {"fin_fe1", &ctx->coop.fin_fe1},
              {"fin_fe2", &ctx->coop.fin_fe2},           {"pset_prep", &ctx->coop.pset_prep},
              {"fin_fe2_w2", &ctx->coop.fin_fe2_w2},
              {"pset_dbl_all", &ctx->coop.pset_dbl_all}, {"pset_add_x", &ctx->coop.pset_add_x},
              {"pset_phase2", &ctx->coop.pset_phase2},
              {"pset_norm2", &ctx->coop.pset_norm2},     {"pset_affine2", &ctx->coop.pset_affine2},
              {"pset_ml2", &ctx->coop.pset_ml2},         {"pset_ml2_w2", &ctx->coop.pset_ml2_w2},
              {"pset_xchain", &ctx->coop.pset_xchain},
              {"ml1_1", &ctx->coop.ml1_1},
              {"ml1_2", &ctx->coop.ml1_2}};
  ctx->coop_progs = new std::vector<std::pair<std::string, CoopProg>>();
  ctx->coop_frames = new std::vector<uint32_t>();
  for (uint32_t k = 0; k < h.n_progs; ++k) {
    CoopProgEntry e;
    memcpy(&e, buf.data() + progs_off + k * sizeof(e), sizeof(e));
    e.name[31] = 0;
    ctx->coop_progs->push_back({std::string(e.name), CoopProg{e.first, e.n_steps}});
    ctx->coop_frames->push_back(e.frame);
  }
  // packed programs (tools/gen_pset.py S = 2, 3): pset{S}_{prep, dbl_all, add_x, ...}
  std::vector<std::pair<std::string, CoopProg*>> want_packed;
  for (int S = 2; S <= 3; ++S) {
    CoopPsetN& pn = ctx->coop.packed[S - 2];
    const std::string pre = "pset" + std::to_string(S) + "_";
    want_packed.push_back({pre + "prep", &pn.prep});
    want_packed.push_back({pre + "dbl_all", &pn.dbl_all});
    want_packed.push_back({pre + "add_x", &pn.add_x});
    want_packed.push_back({pre + "phase2", &pn.phase2});
    want_packed.push_back({pre + "norm2", &pn.norm2});
    want_packed.push_back({pre + "affine2", &pn.affine2});
    want_packed.push_back({pre + "ml2", &pn.ml2});
  }
  for (auto& wp : want_packed) {
    bool found = false;
    for (auto& e : *ctx->coop_progs)
      if (e.first == wp.first) {
        *wp.second = e.second;
        found = true;
      }
    if (!found) {
      snprintf(ctx->err, sizeof(ctx->err), "%s: program %s missing", path.c_str(), wp.first.c_str());
      return -1;
    }
  }
  for (auto& w : want) {
    bool found = false;
    for (uint32_t k = 0; k < h.n_progs; ++k) {
      CoopProgEntry e;
      memcpy(&e, buf.data() + progs_off + k * sizeof(e), sizeof(e));
      if (strncmp(e.name, w.name, sizeof(e.name)) == 0) {
        w.dst->first = e.first;
        w.dst->n = e.n_steps;
        found = true;
      }
    }
    if (!found) {
      snprintf(ctx->err, sizeof(ctx->err), "%s: program %s missing", path.c_str(), w.name);
      return -1;
    }
  }
  // kernels take the struct by pointer (its ~370 bytes by value, next to PipeBufs, made
  // the cooperative kernels' arguments ~830 bytes)
  HIPC(ctx, hipMemcpy((void*)ctx->coop.dev, &ctx->coop, sizeof(CoopEnv), hipMemcpyHostToDevice));
  return 0;
}

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------
// sets of the verify calls running now, over every context of the process (the Miller
// loops pick their shape by it: kernels/k_mlq.hip launch_k_mlqf)
static std::atomic<uint64_t> g_sets_in_flight{0};
uint64_t bls_sets_in_flight() { return g_sets_in_flight.load(std::memory_order_relaxed); }

// ---------------------------------------------------------------------------
// Scratch admission.  The HIP runtime backs every hardware queue with private-segment
// (scratch) memory for a full device of the deepest kernel dispatched on it, and past
// ~8 GiB over the queues in use it aborts them with HSA_STATUS_ERROR_OUT_OF_RESOURCES:
// every call in flight in the process fails and later calls too
// (profiles/r03_scratch_out_of_resources.txt; 16 queues at 464 MiB ran, 16 at 520 MiB
// and 20 at 456 MiB aborted).  So a context is admitted only while the queues its
// contexts map onto, times the deepest verify-path kernel's reservation (baked at build
// time from the kernels' resource usage, lodestar_amd/build.py), fit a budget; otherwise
// bls_gpu_init_priority returns BLS_ERR_ADMISSION with a message, as the reference's pool
// records a worker that failed to start (multithread/index.ts:221-229) and fails queued
// work only when every worker failed (:247-253).
//   queues in use: HIP maps a process's streams of one priority onto at most
//   GPU_MAX_HW_QUEUES hardware queues (default 4), per priority level.
// ---------------------------------------------------------------------------
#ifndef BLS_SCRATCH_PER_QUEUE
#define BLS_SCRATCH_PER_QUEUE 0ull  // set by lodestar_amd/build.py (-D); 0 = unknown (no limit)
#endif
#ifndef BLS_SCRATCH_WORST_KERNEL
#define BLS_SCRATCH_WORST_KERNEL "unknown"
#endif
#define BLS_SCRATCH_BUDGET_DEFAULT (6ull << 30)  // 75 % of the ~8 GiB abort point

namespace {
std::mutex g_adm_mu;
constexpr int ADM_MAX_DEV = 64;
uint32_t g_adm_normal[ADM_MAX_DEV], g_adm_high[ADM_MAX_DEV];
std::atomic<uint64_t> g_adm_budget_override{0};
thread_local char g_init_err[512];

// The HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues per
// priority (HIP's default 4), read once when the runtime initialises, and streams
// sharing a queue serialise: 12 contexts x 22 calls give 2.27M sets/s on 4 queues
// against 3.42M on 16 and 3.65M on 24 (bench.py hw_queues_4 / hw_queues_16,
// profiles/r05_bench_first.json).  The library never writes the environment by itself
// (a load-time setenv would race getenv on a multithreaded host's other threads and leak
// into every child process): the host asks with bls_gpu_request_hw_queues before any
// HIP use (the Python and JS wrappers do as they load the library), and the library
// records what the runtime really got -- the variable's value when the runtime
// initialised, if that happened under this library's first context, or "unknown" when
// another component of the process had initialised HIP first (hw_queues_known = 0 in
// bls_admission, and one warning on stderr when the runtime then most likely kept
// HIP's 4 queues).
namespace {
// the render / KFD device is open once the ROCm runtime initialised in this process
bool hip_runtime_up() {
  char path[64], target[64];
  for (int fd = 0; fd < 4096; ++fd) {
    snprintf(path, sizeof(path), "/proc/self/fd/%d", fd);
    const ssize_t n = readlink(path, target, sizeof(target) - 1);
    if (n <= 0) continue;
    target[n] = 0;
    if (strcmp(target, "/dev/kfd") == 0) return true;
  }
  return false;
}

uint32_t parse_hwq(const char* e) {
  const long v = e && *e ? strtol(e, nullptr, 10) : 0;
  return v > 0 ? (uint32_t)v : 4u;
}

bool g_hip_up_at_load = false;  // HIP was initialised before this library loaded
// the runtime's queue count: fixed at this library's first context (when the runtime
// came up under it, hwq_known = 1) or guessed from the environment (hwq_known = 0)
std::once_flag g_hwq_once;
uint32_t g_hwq_effective = 0;
bool g_hwq_known = false;

__attribute__((constructor)) void bls_record_runtime_state() { g_hip_up_at_load = hip_runtime_up(); }

// called by bls_gpu_init_priority before its first HIP call (g_adm_mu held)
void note_runtime_queues() {
  std::call_once(g_hwq_once, [] {
    const bool up = g_hip_up_at_load || hip_runtime_up();
    const char* e = getenv("GPU_MAX_HW_QUEUES");
    g_hwq_effective = parse_hwq(e);
    g_hwq_known = !up;
    if (up && !(e && *e))
      fprintf(stderr,
              "lodestar_bls: warning: the HIP runtime was initialised before this library's first context, "
              "with GPU_MAX_HW_QUEUES unset: its streams share HIP's default 4 hardware queues per priority, so "
              "more than 4 verifier contexts serialise (set GPU_MAX_HW_QUEUES before the process's first HIP "
              "call, or call bls_gpu_request_hw_queues first; INTEGRATION.md section 4)\n");
  });
}
}  // namespace

uint32_t hw_queues_env() {
  if (g_hwq_effective) return g_hwq_effective;
  return parse_hwq(getenv("GPU_MAX_HW_QUEUES"));
}

uint64_t scratch_budget() {
  const uint64_t o = g_adm_budget_override.load();
  if (o) return o;
  const char* e = getenv("BLS_SCRATCH_BUDGET_MIB");
  const unsigned long long v = e && *e ? strtoull(e, nullptr, 10) : 0ull;
  return v ? (uint64_t)v << 20 : BLS_SCRATCH_BUDGET_DEFAULT;
}

void init_fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void init_fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_init_err, sizeof(g_init_err), fmt, ap);
  va_end(ap);
}
}  // namespace

extern "C" {

int bls_scratch_plan(uint32_t n_normal, uint32_t n_high, uint32_t hw_queues, bls_admission* out) {
  bls_admission a;
  memset(&a, 0, sizeof(a));
  a.contexts_normal = n_normal;
  a.contexts_high = n_high;
  a.hw_queues = hw_queues ? hw_queues : hw_queues_env();
  a.hw_queues_known = hw_queues ? 1u : (g_hwq_effective ? (g_hwq_known ? 1u : 0u) : 2u);
  a.queues_in_use = (n_normal < a.hw_queues ? n_normal : a.hw_queues) + (n_high < a.hw_queues ? n_high : a.hw_queues);
  a.scratch_per_queue = BLS_SCRATCH_PER_QUEUE;
  a.scratch_reserved = (uint64_t)a.queues_in_use * a.scratch_per_queue;
  a.scratch_budget = scratch_budget();
  if (out) *out = a;
  return a.scratch_reserved <= a.scratch_budget ? 0 : BLS_ERR_ADMISSION;
}

const char* bls_scratch_worst_kernel(void) { return BLS_SCRATCH_WORST_KERNEL; }

int bls_gpu_request_hw_queues(uint32_t n) {
  if (n == 0) return -2;
  const char* e = getenv("GPU_MAX_HW_QUEUES");
  if (e && *e) return 1;  // the host's own choice stands
  if (g_hip_up_at_load || g_hwq_effective || hip_runtime_up()) return 2;  // too late: the runtime has its count
  char v[16];
  snprintf(v, sizeof(v), "%u", n);
  return setenv("GPU_MAX_HW_QUEUES", v, 0) == 0 ? 0 : -1;
}

int bls_gpu_admission(int device, bls_admission* out) {
  if (device < 0 || device >= ADM_MAX_DEV) return -2;
  std::lock_guard<std::mutex> g(g_adm_mu);
  return bls_scratch_plan(g_adm_normal[device], g_adm_high[device], 0, out);
}

void bls_gpu_set_scratch_budget(uint64_t bytes) { g_adm_budget_override.store(bytes); }

const char* bls_gpu_init_error(void) { return g_init_err; }

int bls_gpu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int bls_gpu_init(int device, bls_gpu_ctx** out) { return bls_gpu_init_priority(device, BLS_PRIORITY_NORMAL, out); }

int bls_gpu_init_priority(int device, int priority, bls_gpu_ctx** out) {
  if (!out) return -2;
  *out = nullptr;
  g_init_err[0] = 0;
  if (device < 0 || device >= ADM_MAX_DEV) {
    init_fail("bls_gpu_init: device %d out of range", device);
    return -2;
  }
  const bool high = priority == BLS_PRIORITY_HIGH;
  {
    // admit first: a refused context never creates its stream (no queue, no reservation)
    std::lock_guard<std::mutex> g(g_adm_mu);
    note_runtime_queues();  // before this library's first HIP call
    bls_admission a;
    const uint32_t nn = g_adm_normal[device] + (high ? 0u : 1u), nh = g_adm_high[device] + (high ? 1u : 0u);
    if (bls_scratch_plan(nn, nh, 0, &a) != 0) {
      init_fail("BLS_ERR_ADMISSION: a %s-priority context on device %d would map %u normal + %u high-priority "
                "contexts onto %u hardware queues (GPU_MAX_HW_QUEUES=%u), reserving %llu MiB of scratch "
                "(%llu MiB per queue for %s) > the %llu MiB budget ($BLS_SCRATCH_BUDGET_MIB); close a context or "
                "lower the context count",
                high ? "high" : "normal", device, nn, nh, a.queues_in_use, a.hw_queues,
                (unsigned long long)(a.scratch_reserved >> 20), (unsigned long long)(a.scratch_per_queue >> 20),
                BLS_SCRATCH_WORST_KERNEL, (unsigned long long)(a.scratch_budget >> 20));
      return BLS_ERR_ADMISSION;
    }
    if (high) ++g_adm_high[device];
    else ++g_adm_normal[device];
  }
  bls_gpu_ctx* ctx = new bls_gpu_ctx();
  memset(ctx, 0, sizeof(*ctx));
  ctx->mu = new std::mutex();
  ctx->device = device;
  ctx->admitted = high ? 2 : 1;
  // every failure below releases what was made through bls_gpu_close (it tolerates
  // members that were never created) and leaves its message for bls_gpu_init_error
  auto fail = [&](const char* what, hipError_t e) {
    init_fail("bls_gpu_init: %s: %s", what, hipGetErrorString(e));
    bls_gpu_close(ctx);
    return -1;
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail("hipSetDevice", e);
  int prio_lo = 0, prio_hi = 0;  // HIP: numerically lower = higher priority
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if ((e = hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, high ? prio_hi : prio_lo)) != hipSuccess)
    return fail("hipStreamCreateWithPriority", e);
  if ((e = hipEventCreate(&ctx->ev0)) != hipSuccess || (e = hipEventCreate(&ctx->ev1)) != hipSuccess)
    return fail("hipEventCreate", e);
  for (int i = 0; i < 9; ++i)
    if ((e = hipEventCreate(&ctx->ev[i])) != hipSuccess) return fail("hipEventCreate", e);
  if ((e = hipEventCreateWithFlags(&ctx->ev_wait, hipEventDisableTiming)) != hipSuccess)
    return fail("hipEventCreateWithFlags", e);
  if (load_coop_tables(ctx) != 0) {
    init_fail("bls_gpu_init: %s", ctx->err);
    bls_gpu_close(ctx);
    return -1;
  }
  if ((e = hipMalloc(&ctx->first_bad, 2 * sizeof(uint32_t))) != hipSuccess ||
      (e = hipMemset(ctx->first_bad, 0xFF, 2 * sizeof(uint32_t))) != hipSuccess)
    return fail("first_bad", e);
  // the MSM's bucket counters and tickets: zeroed here once, then reset by the kernels'
  // last workgroups (and re-zeroed after a failed call, verify_impl)
  if ((e = hipMalloc(&ctx->msm_state, sizeof(uint32_t) * MSM_STATE_WORDS)) != hipSuccess ||
      (e = hipMemset(ctx->msm_state, 0, sizeof(uint32_t) * MSM_STATE_WORDS)) != hipSuccess)
    return fail("msm_state", e);
  if ((e = hipMalloc(&ctx->cm_dev, sizeof(CommitteeGroupDev) * BLS_COMMITTEE_GROUPS)) != hipSuccess ||
      (e = hipMemset(ctx->cm_dev, 0, sizeof(CommitteeGroupDev) * BLS_COMMITTEE_GROUPS)) != hipSuccess)
    return fail("committee groups", e);
  ctx->cm = committee_slots_new();
  pk_table_new(ctx);
  *out = ctx;
  return 0;
}

void bls_gpu_close(bls_gpu_ctx* ctx) {
  if (!ctx) return;
  ctx->mu->lock();  // wait for a call in flight on another thread
  ctx->mu->unlock();
  if (ctx->admitted) {
    std::lock_guard<std::mutex> g(g_adm_mu);
    if (ctx->admitted == 2) --g_adm_high[ctx->device];
    else --g_adm_normal[ctx->device];
    ctx->admitted = 0;
  }
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  delete ctx->cm;  // every group's allocation
  if (ctx->cm_dev) (void)hipFree(ctx->cm_dev);
  pk_table_release(ctx);  // the table goes with its last context
  if (ctx->dev_ws) (void)hipFree(ctx->dev_ws);
  if (ctx->host_stage) (void)hipHostFree(ctx->host_stage);
  if (ctx->host_res) (void)hipHostFree(ctx->host_res);
  if (ctx->first_bad) (void)hipFree(ctx->first_bad);
  if (ctx->msm_state) (void)hipFree(ctx->msm_state);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->ev_wait) (void)hipEventDestroy(ctx->ev_wait);
  for (int i = 0; i < 9; ++i)
    if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
  if (ctx->coop_dev) (void)hipFree(ctx->coop_dev);
  delete ctx->coop_progs;
  delete ctx->coop_frames;
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx->mu;
  delete ctx;
}

const char* bls_gpu_last_error(const bls_gpu_ctx* ctx) { return ctx ? ctx->err : "no context"; }

// ---------------------------------------------------------------------------
// comb rows of the table's keys (curve.hpp g1_comb_build)
// ---------------------------------------------------------------------------
static bool pk_comb_on() {
  static const bool on = [] {
    const char* e = getenv("BLS_PK_COMB");
    return !(e && *e && atoi(e) == 0);
  }();
  return on;
}

// keys whose rows one table may hold: $BLS_PK_COMB_MAX_MB of comb memory (default 4096,
// about 2.9M keys at 1,440 B each); keys past it keep the GLV chain
static uint32_t pk_comb_max_keys() {
  uint64_t mb = 4096;
  const char* e = getenv("BLS_PK_COMB_MAX_MB");
  if (e && *e) mb = strtoull(e, nullptr, 10);
  const uint64_t keys = (mb << 20) / (sizeof(Fp) * G1_COMB_WORDS);
  return keys > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)keys;
}

// device memory as bls/pk_table.hpp sees it
static void* pk_mem_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes) == hipSuccess) return p;
  (void)hipGetLastError();
  return nullptr;
}
static void pk_mem_free(void* p) { (void)hipFree(p); }
static bool pk_mem_copy(void* dst, const void* src, size_t bytes, void* stream) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess;
}
static bool pk_mem_sync(void* stream) { return hipStreamSynchronize((hipStream_t)stream) == hipSuccess; }
static const PkMem g_pk_mem = {pk_mem_alloc, pk_mem_free, pk_mem_copy, pk_mem_sync};

static Fp* g1_comb_make(bls_gpu_ctx* ctx);

// a context's own table, empty (at creation); $BLS_PK_COMB decides whether it grows rows
static void pk_table_new(bls_gpu_ctx* ctx) {
  const bool comb_off = !pk_comb_on();
  auto t = std::make_shared<PkTable>(&g_pk_mem, ctx->device, sizeof(G1A), sizeof(Fp) * G1_COMB_WORDS, comb_off);
  if (!comb_off) t->set_g1_comb(g1_comb_make(ctx));
  t->attach();
  ctx->pkt = new std::shared_ptr<PkTable>(std::move(t));
}

// the context lets go of its table: the last one out frees it (no table mutex is held)
static void pk_table_release(bls_gpu_ctx* ctx) {
  if (!ctx->pkt) return;
  (*ctx->pkt)->detach();
  delete ctx->pkt;
  ctx->pkt = nullptr;
}

// The table as one call sees it from its first kernel to its last stream synchronisation.
struct PkView {
  PkSnapshot snap;
  const G1A* table() const { return (const G1A*)snap.gen->table_p(); }
  const Fp* comb() const { return (const Fp*)snap.gen->comb_p(); }
  const uint8_t* comb_ok() const { return snap.gen->comb_ok_p(); }
};
static PkView pk_snapshot(const bls_gpu_ctx* ctx) { return PkView{(*ctx->pkt)->snapshot()}; }

// The generator's rows, by the builder the table's keys get (one lane); a failure only
// leaves the per-set path's RG lanes on the GLV chain.
static Fp* g1_comb_make(bls_gpu_ctx* ctx) {
  const size_t off_tmp = 256, off_ok = off_tmp + sizeof(G1J) * G1_COMB_ROWS;
  static_assert(sizeof(G1A) <= 256, "the key sits before the builder's workspace");
  uint8_t* buf = nullptr;
  Fp* rows = nullptr;
  const G1A g = g1_generator();
  uint8_t ok = 0;
  const bool good =
      hipMalloc(&buf, off_ok + 16) == hipSuccess && hipMalloc(&rows, sizeof(Fp) * G1_COMB_WORDS) == hipSuccess &&
      hipMemcpy(buf, &g, sizeof(g), hipMemcpyHostToDevice) == hipSuccess &&
      launch_k_comb_build((const G1A*)buf, 1, (G1J*)(buf + off_tmp), rows, buf + off_ok, ctx->stream) == hipSuccess &&
      hipStreamSynchronize(ctx->stream) == hipSuccess &&
      hipMemcpy(&ok, buf + off_ok, 1, hipMemcpyDeviceToHost) == hipSuccess;
  if (buf) (void)hipFree(buf);
  if (good && ok) return rows;
  (void)hipGetLastError();
  if (rows) (void)hipFree(rows);
  return nullptr;
}

// rows and comb_ok of the keys [from, to) of a generation, in batches that bound the
// builder's workspace (15 Jacobian entries per key, freed afterwards); false: give the
// comb up (PkTable::append)
static bool comb_build(bls_gpu_ctx* ctx, const PkGen& gen, uint32_t from, uint32_t to) {
  const uint32_t BATCH = 1u << 16;
  const uint32_t todo = to - from;
  const G1A* table = (const G1A*)gen.table_p();
  Fp* comb = (Fp*)gen.comb_p();
  G1J* tmp = nullptr;
  bool good = hipMalloc(&tmp, sizeof(G1J) * G1_COMB_ROWS * (size_t)(todo < BATCH ? todo : BATCH)) == hipSuccess;
  for (uint32_t at = from; good && at < to; at += BATCH) {
    const uint32_t m = to - at < BATCH ? to - at : BATCH;
    good = launch_k_comb_build(table + at, m, tmp, comb + (size_t)G1_COMB_WORDS * at, gen.comb_ok_p() + at,
                               ctx->stream) == hipSuccess;
  }
  good = good && hipStreamSynchronize(ctx->stream) == hipSuccess;
  if (tmp) (void)hipFree(tmp);
  if (!good) (void)hipGetLastError();
  return good;
}

// The load runs on the calling context's stream and workspace, under its table's loader
// mutex (PkTable::append: decode, wait, rows, wait, and only then the new size for every
// context that shares the table).
int64_t bls_gpu_load_pubkeys(bls_gpu_ctx* ctx, const uint8_t* pks, uint32_t n, uint32_t pk_len, int32_t* codes) {
  CTX_LOCK(ctx);
  if (pk_len != 48 && pk_len != 96) {
    snprintf(ctx->err, sizeof(ctx->err), "pk_len must be 48 or 96");
    return -1;
  }
  HIPC(ctx, hipSetDevice(ctx->device));
  const size_t in_bytes = (size_t)pk_len * n;
  // all or nothing: a key that does not decode leaves the table as it was, so table
  // indices (validator indices) stay aligned across calls
  auto decode = [&](uint8_t* dst) -> int {
    std::vector<int32_t> host_codes(n);
    uint8_t* d_in = nullptr;
    int32_t* d_codes = nullptr;
    OneShot run(ctx);
    if (run.carve([&](Carver& c) { c.buf(d_in, in_bytes).buf(d_codes, n); }) || ensure_host(ctx, run.bytes)) return -2;
    HIPC(ctx, hipMemcpyAsync(d_in, pks, in_bytes, hipMemcpyHostToDevice, run.s));
    HIPC(ctx, launch_k_load_pubkeys(d_in, n, pk_len, (G1A*)dst, d_codes, run.s));
    HIPC(ctx, hipMemcpyAsync(host_codes.data(), d_codes, sizeof(int32_t) * n, hipMemcpyDeviceToHost, run.s));
    if (run.finish()) return -1;
    if (codes) memcpy(codes, host_codes.data(), sizeof(int32_t) * n);
    for (uint32_t i = 0; i < n; ++i)
      if (host_codes[i] != 0) return 1;
    return 0;
  };
  auto build = [&](const PkGen& gen, uint32_t from, uint32_t to) { return comb_build(ctx, gen, from, to); };
  bool decode_err = false;  // (the decode left its own message)
  auto decode_step = [&](uint8_t* dst) {
    const int rc = decode(dst);
    decode_err = rc < 0;
    return rc;
  };
  const char* what = "load";
  const int64_t r = (*ctx->pkt)->append(n, pk_comb_max_keys(), ctx->stream, decode_step, build, &what);
  if (r < 0 && !decode_err) {
    (void)hipGetLastError();
    snprintf(ctx->err, sizeof(ctx->err), "bls_gpu_load_pubkeys: %s failed", what);
  }
  return r;
}

// ctx leaves its (empty) table for the one `with` uses.  Both contexts' mutexes are held
// (std::lock: two opposite calls do not deadlock), so neither has a call in flight and
// neither's table pointer moves meanwhile.
extern "C" int bls_gpu_share_pubkeys(bls_gpu_ctx* ctx, bls_gpu_ctx* with) {
  if (!ctx || !with || ctx == with) {
    if (ctx) {
      CTX_LOCK(ctx);
      snprintf(ctx->err, sizeof(ctx->err), "bls_gpu_share_pubkeys: %s",
               with ? "a context cannot share with itself" : "no context to share with");
    }
    return -2;
  }
  std::shared_ptr<PkTable> old;  // released after the mutexes
  {
    std::unique_lock<std::mutex> a(*ctx->mu, std::defer_lock), b(*with->mu, std::defer_lock);
    std::lock(a, b);
    if (*ctx->pkt == *with->pkt) return 0;
    if (ctx->device != with->device) {
      snprintf(ctx->err, sizeof(ctx->err), "bls_gpu_share_pubkeys: the contexts are on devices %d and %d",
               ctx->device, with->device);
      return -2;
    }
    const uint32_t held = (*ctx->pkt)->size();
    if (held != 0) {
      snprintf(ctx->err, sizeof(ctx->err), "bls_gpu_share_pubkeys: the context already holds %u keys", held);
      return -2;
    }
    (*ctx->pkt)->detach();
    old = std::move(*ctx->pkt);
    *ctx->pkt = *with->pkt;
    (*ctx->pkt)->attach();
  }
  (void)hipSetDevice(ctx->device);
  old.reset();
  return 0;
}

extern "C" int bls_gpu_pubkeys_info(bls_gpu_ctx* ctx, bls_pubkeys_info* out) {
  if (!ctx || !out) return -2;
  CTX_LOCK(ctx);
  const PkInfo i = (*ctx->pkt)->info();
  out->table_id = i.table_id;
  out->n_keys = i.n_keys;
  out->capacity = i.capacity;
  out->comb_keys = i.comb_keys;
  out->n_contexts = i.n_contexts;
  out->device_bytes = i.device_bytes;
  return 0;
}

int bls_gpu_validate_pubkeys(bls_gpu_ctx* ctx, const uint8_t* pks, uint32_t n, uint32_t pk_len, int32_t* codes) {
  CTX_LOCK(ctx);
  if ((pk_len != 48 && pk_len != 96) || !codes) {
    snprintf(ctx->err, sizeof(ctx->err), "pk_len must be 48 or 96 and codes non-null");
    return -2;
  }
  if (n == 0) return 0;
  HIPC(ctx, hipSetDevice(ctx->device));
  const size_t in_bytes = (size_t)pk_len * n;
  uint8_t* d_in = nullptr;
  int32_t* d_codes = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { c.buf(d_in, in_bytes).buf(d_codes, n); })) return -1;
  HIPC(ctx, hipMemcpyAsync(d_in, pks, in_bytes, hipMemcpyHostToDevice, run.s));
  HIPC(ctx, launch_k_validate_pubkeys(d_in, n, pk_len, d_codes, run.s));
  HIPC(ctx, hipMemcpyAsync(codes, d_codes, sizeof(int32_t) * n, hipMemcpyDeviceToHost, run.s));
  return run.finish();
}

// ---------------------------------------------------------------------------
// committee groups (bls/committee.hpp)
// ---------------------------------------------------------------------------
static CommitteeSlots* committee_slots_new() { return new CommitteeSlots(&g_pk_mem, sizeof(G1J)); }

extern "C" int bls_gpu_set_committee_group(bls_gpu_ctx* ctx, uint32_t group, uint32_t n, const uint32_t* member_offsets,
                                           const uint32_t* members) {
  if (!ctx) return -2;
  CTX_LOCK(ctx);
  // the table as it is now: append-only, so what is below n stays put under the totals
  const PkView pk = pk_snapshot(ctx);
  if (const int rc = committee_check_group(group, n, member_offsets, members, pk.snap.n, ctx->err, sizeof(ctx->err)))
    return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  const hipStream_t s = ctx->stream;
  const auto upload = [&](void* dst, const void* src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
           hipStreamSynchronize(s) == hipSuccess;  // (the caller's arrays are pageable: done before the return)
  };
  const auto totals = [&](const CommitteeGroupDev& v) {
    return launch_k_committee_totals(v, (G1J*)v.totals, pk.table(), pk.snap.n, s) == hipSuccess &&
           hipStreamSynchronize(s) == hipSuccess;
  };
  const char* what = nullptr;
  // the slot is swapped (and the old allocation freed) only by a set() that succeeded, and
  // the stream is idle under the lock, so no kernel reads the views while they change
  if (ctx->cm->set(group, n, member_offsets, members, upload, totals, &what) != 0) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s);
    snprintf(ctx->err, sizeof(ctx->err), "bls_gpu_set_committee_group: %s failed", what ? what : "a step");
    return -1;
  }
  CommitteeGroupDev views[BLS_COMMITTEE_GROUPS];
  ctx->cm->views(views);
  HIPC(ctx, hipMemcpyAsync(ctx->cm_dev, views, sizeof(views), hipMemcpyHostToDevice, s));
  HIPC(ctx, hipStreamSynchronize(s));
  return 0;
}

extern "C" int bls_gpu_committee_group_info(bls_gpu_ctx* ctx, uint32_t group, bls_committee_info* out) {
  if (!ctx || !out) return -2;
  CTX_LOCK(ctx);
  if (group >= BLS_COMMITTEE_GROUPS) {
    snprintf(ctx->err, sizeof(ctx->err), "committee group %u: only groups 0..%u exist", group,
             BLS_COMMITTEE_GROUPS - 1u);
    return -2;
  }
  *out = ctx->cm->info(group);
  return 0;
}

// $BLS_DEBUG_SYNC: synchronise after every kernel of a verify call and log its name
// and wall time to stderr (a kernel that never finishes is the last name printed)
static void dbg_sync(hipStream_t s, const char* what) {
  if (!knobs().debug_sync) return;
  timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  fprintf(stderr, "[bls sync] %s ...", what);
  fflush(stderr);
  hipError_t e = hipStreamSynchronize(s);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  fprintf(stderr, " %.3f ms %s\n", (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6,
          hipGetErrorString(e));
  fflush(stderr);
}

struct InFlight {
  uint64_t n;
  explicit InFlight(uint64_t k) : n(k) { g_sets_in_flight.fetch_add(n, std::memory_order_relaxed); }
  ~InFlight() { g_sets_in_flight.fetch_sub(n, std::memory_order_relaxed); }
};

static hipError_t pass_wait(bls_gpu_ctx* ctx, hipStream_t s) {
  if (!ctx->wait_block || s != ctx->stream) return hipStreamSynchronize(s);
  hipError_t e = hipEventRecord(ctx->ev_wait, s);
  if (e != hipSuccess) return e;
  const struct timespec nap = {0, 50000};
  while ((e = hipEventQuery(ctx->ev_wait)) == hipErrorNotReady) nanosleep(&nap, nullptr);
  return e;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// The verify pass
// ---------------------------------------------------------------------------
namespace {

// The k_fprod product tree over in[0, m): levels of FPROD_FAN through the two buffers t.
// With `verdict` the levels stop at FPROD_FAN elements and the last launch writes
// FE(product) == 1 there; without it they run down to one element, left at *out.
int fprod_tree(bls_gpu_ctx* ctx, const Fp12* in, uint32_t m, Fp12* const t[2], int32_t* verdict, const Fp12** out,
               hipStream_t s) {
  const uint32_t stop = verdict ? FPROD_FAN : 1u;
  const Fp12* cur = in;
  for (uint32_t lvl = 0; m > stop; ++lvl) {
    HIPC(ctx, launch_k_fprod(cur, m, t[lvl & 1], nullptr, ctx->coop, s)); dbg_sync(s, "k_fprod");
    cur = t[lvl & 1];
    m = (m + FPROD_FAN - 1) / FPROD_FAN;
  }
  if (verdict) {
    HIPC(ctx, launch_k_fprod(cur, m, nullptr, verdict, ctx->coop, s)); dbg_sync(s, "k_fprod verdict");
  }
  if (out) *out = cur;
  return 0;
}

inline hipError_t launch_gsum_level(const PipeBufs& b, const uint32_t* seg, uint32_t n_seg, const G2J* in, G2J* out,
                                    hipStream_t s) {
  return launch_k_gsum(b, seg, n_seg, in, out, s);
}
inline hipError_t launch_gsum_level(const PipeBufs& b, const uint32_t* seg, uint32_t n_seg, const G1J* in, G1J* out,
                                    hipStream_t s) {
  return launch_k_gsum1(b, seg, n_seg, in, out, s);
}

// Run the levels of `p` (seg_dev: its pairs on the device) over the sets b.gsets names, G2
// points by k_gsum or G1 points by k_gsum1; tmp: two point buffers of level-0 size.
// *sums: one point per group, in group order.
template <class P>
int gsum_levels(bls_gpu_ctx* ctx, const PipeBufs& b, const GsumPlan& p, const uint32_t* seg_dev, P* const tmp[2],
                const char* what, const P** sums, hipStream_t s) {
  const P* in = nullptr;
  for (size_t L = 0; L + 1 < p.level_off.size(); ++L) {
    const uint32_t beg = p.level_off[L], n_seg = p.level_off[L + 1] - beg;
    HIPC(ctx, launch_gsum_level(b, seg_dev + 2 * beg, n_seg, in, tmp[L & 1], s)); dbg_sync(s, what);
    in = tmp[L & 1];
  }
  *sums = in;
  return 0;
}

// what an entry point asks of the pass
struct PassArgs {
  int32_t* verdicts;
  bls_stats* stats;
  uint32_t scalar_base;
  uint8_t* partial_out;  // non-null: the Miller-loop partial of one shard (bls_gpu_partial)
  int32_t* partial_status;
  uint32_t* partial_err;
  const std::vector<uint32_t>* req_bounds;  // verify_many: the messages' first requests
  const SameMsgPlan* sm;                    // verify_same_message: its own plan
  // verify_deposits: the caller's arrays.  The batch of such a pass is n one-set batchable
  // requests with neither keys nor messages on the host: k_deposit makes both
  const bls_deposit_batch* dep;
  // the call's snapshot of the pubkey table (nullptr for a deposit call: no table)
  const PkView* pk;
  // verify_committees: which sets name a committee, and their bits (nullptr: none does)
  const bls_committee_sets* cs;
  // verify_spans: which sets are spans of committees, and their fields (nullptr: none is)
  const bls_span_sets* ss;
};

// One verify call's pass over the device: shape and plans fixed at construction, buffers
// carved by stage_inputs, then the stages in the order verify_body calls them.  Every
// stage returns 0 or the call's error code (ctx->err set).
struct VerifyPass {
  bls_gpu_ctx* const ctx;
  const bls_batch* const in;
  const PassArgs a;
  const hipStream_t s;
  PassPlans pl;
  const PassShape sh;
  const BatchPlan& plan;

  // ---- buffers (carve / carve_res)
  PipeBufs b;
  GroupBufs g;
  MsmBufs msm;
  DepositBufs dep;
  size_t input_end = 0;                  // [0, input_end) of the carve is the mapped staging area
  Fp12* ptree[2] = {nullptr, nullptr};   // product-tree levels (partial mode, merged check)
  int32_t* merged_ok = nullptr;          // FE(prod f_i) == 1 of the merged check
  uint32_t* gsets_dev = nullptr;         // group-sum plans (aggregated-signature path)
  uint32_t* gseg_dev = nullptr;
  uint32_t* tseg_dev = nullptr;          // the merged signature sum's plan
  G2J* gtmp[2] = {nullptr, nullptr};
  G1J* utmp[2] = {nullptr, nullptr};
  uint32_t *unit_rep_dev = nullptr, *ugsets_dev = nullptr, *useg_dev = nullptr;  // Miller-loop units
  uint32_t* own_sets_dev = nullptr;  // the individually verified sets' own Miller loops + the requests' sums (one launch)
  Fp12* fe_save = nullptr;

  // ---- what the stages leave for the later ones
  bool rs_done;          // the per-set RS = [r] sig (chain CH_RS) exist (ensure_rs)
  uint32_t pass_pl = 0;  // the first pass's items per k_mlf lane
  bool msm_overlapped = false;  // the first pass ran the Pippenger sum inside its Miller-loop launches
  std::vector<int32_t> chunk_ok, merged_status;
  int32_t merged_verdict = 0;
  uint32_t flagged = 0;
  bool merged_pass = false, chunk_fe_kept = false;
  IndivPlan iv;
  bool gsums = false;   // group sums: the group tests pair one signature sum per test (group_sums)
  uint32_t n_sum = 0;   // requests pairing their own signature sum: iv.reqs[0, n_sum)
  std::vector<int32_t> indiv_verdict;
  std::vector<uint32_t> bits_list;  // the committee sets (k_pk_bits), a.cs
  std::vector<uint32_t> span_list;  // the span sets (k_pk_span), a.ss
  FoldPlan fold;        // outlive the kernels that read them from the staging area
  GsumPlan indiv_gsum;

  VerifyPass(bls_gpu_ctx* c, const bls_batch* batch, const PassArgs& args)
      : ctx(c), in(batch), a(args), s(c->stream),
        sh(plan_pass(batch, PassAsk{args.partial_out != nullptr, args.sm, args.dep != nullptr, args.req_bounds},
                     PassEnv{c->debug_flags, c->last_merged_failed, bls_sets_in_flight()}, knobs(), pl)),
        plan(*pl.plan),
        rs_done(!sh.use_msm), chunk_ok(sh.n_chunks + 1, 0), merged_status(sh.merged ? sh.R : 0, 0) {
    memset(&b, 0, sizeof(b));
    memset(&g, 0, sizeof(g));
    memset(&msm, 0, sizeof(msm));
    memset(&dep, 0, sizeof(dep));
    if (a.cs)
      for (uint32_t i = 0; i < sh.n; ++i)
        if (a.cs->set_committee[i] != BLS_SET_NO_COMMITTEE) bits_list.push_back(i);
    if (a.ss)
      for (uint32_t i = 0; i < sh.n; ++i)
        if (a.ss->set_span_off[i + 1] != a.ss->set_span_off[i]) span_list.push_back(i);
  }

  // ---- workspace: inputs first (they live in the mapped staging area), then intermediates.
  // Runs once without a base for the sizes and once for the pointers.
  void carve(Carver& c) {
    const uint32_t n = sh.n, R = sh.R, n_chunks = sh.n_chunks;
    const bool sigagg = sh.sigagg, units = sh.use_units, gt = sh.gt_possible;
    b.req_off = c.take<uint32_t>(R + 1);
    b.chunk_off = c.take<uint32_t>(n_chunks + 1);
    b.chunk_reqs = c.take<uint32_t>(plan.chunk_reqs.size());
    b.seed = c.take<uint32_t>(8);
    b.pubkeys = in->set_pk_offsets || sh.dep ? nullptr : c.take<uint8_t>(96ull * n);
    b.set_pk_off = in->set_pk_offsets ? c.take<uint32_t>(n + 1) : nullptr;
    b.pk_idx = in->set_pk_offsets ? c.take<uint32_t>(sh.n_pk_idx) : nullptr;
    b.agg_sets = pl.agg_list.empty() ? nullptr : c.take<uint32_t>(pl.agg_list.size());
    if (!bits_list.empty()) {
      b.set_committee = c.take<uint32_t>(n);
      b.set_bits_off = c.take<uint32_t>(n + 1);
      b.bits = c.take<uint8_t>(a.cs->set_bits_off[n]);
      b.bits_sets = c.take<uint32_t>(bits_list.size());
    }
    if (!span_list.empty()) {
      b.set_span_off = c.take<uint32_t>(n + 1);
      b.span_refs = c.take<uint32_t>(a.ss->set_span_off[n]);
      b.set_bits_off = c.take<uint32_t>(n + 1);
      b.bits = c.take<uint8_t>(a.ss->set_bits_off[n]);
      b.span_sets = c.take<uint32_t>(span_list.size());
    }
    b.msgs = sh.dep ? nullptr : c.take<uint8_t>(32ull * n);  // (a deposit call: device memory, below)
    if (sh.dep) {
      dep.pubkeys48 = c.take<uint8_t>(48ull * n);
      dep.wc = c.take<uint8_t>(32ull * n);
      dep.amounts = c.take<uint8_t>(8ull * n);
      dep.domain = c.take<uint8_t>(32);
    }
    b.msg_uniq = sh.dedup ? c.take<uint32_t>(sh.n_uniq) : nullptr;
    b.msg_rep = sh.dedup ? c.take<uint32_t>(n) : nullptr;
    b.sigs = c.take<uint8_t>(96ull * n);
    b.sig_lens = in->signature_lens ? c.take<uint32_t>(n) : nullptr;
    b.indiv_reqs = c.take<uint32_t>(R);
    g.off = c.take<uint32_t>(gt ? sh.grp_cap + 1 : 0);
    g.members = c.take<uint32_t>(sh.grp_mem_cap);
    g.ref = c.take<uint32_t>(gt ? sh.grp_cap : 0);
    own_sets_dev = sigagg ? c.take<uint32_t>((size_t)n + R) : nullptr;
    b.fold_groups = c.take<uint32_t>(2ull * (n / BLS_FOLD1 + R + 1) + 2ull * (n / BLS_FOLD + R + 1));
    b.ml_dom = sh.ml_shared ? c.take<uint32_t>(sh.indiv_vbase) : nullptr;
    gsets_dev = sigagg ? c.take<uint32_t>(n) : nullptr;
    gseg_dev = sigagg ? c.take<uint32_t>(sh.gseg_cap) : nullptr;
    tseg_dev = sh.use_total ? c.take<uint32_t>(pl.total_gsum.seg.size()) : nullptr;
    if (units) {
      b.set_unit = c.take<uint32_t>(n);
      unit_rep_dev = c.take<uint32_t>(sh.n_units);
      b.unit_off = c.take<uint32_t>(n_chunks + 1);
      ugsets_dev = sh.smsum ? nullptr : c.take<uint32_t>(pl.units.members.size());
      useg_dev = sh.smsum ? nullptr : c.take<uint32_t>(pl.unit_gsum.seg.size());
    }
    input_end = c.off;
    if (sh.dep) b.msgs = dep.roots = c.take<uint8_t>(32ull * n);  // written by k_deposit
    b.sig = c.take<G2A>(n);
    b.sig_status = c.take<int32_t>(n);
    b.pk = c.take<G1J>(n);
    b.pk_status = c.take<int32_t>(n);
    b.pk_inf = sh.partial ? c.take<uint8_t>(n) : nullptr;
    b.q = c.take<Fp>(8ull * n);
    b.chain = sigagg ? c.take<Fp>((size_t)CHAIN_WORDS * sh.n_total) : nullptr;
    b.chain_live = sigagg ? c.take<uint32_t>(sh.n_total) : nullptr;
    b.chain_st = sigagg ? c.take<uint8_t>(4ull * n) : nullptr;
    b.rtab2 = sigagg ? c.take<G2J>(15ull * n) : nullptr;
    b.rtab1 = c.take<G1J>((sigagg ? 15ull : 30ull) * n);
    b.rpts = sigagg ? nullptr : c.take<G1J>(2ull * n);
    gtmp[0] = sigagg ? c.take<G2J>(sh.gtmp_cap) : nullptr;
    gtmp[1] = sigagg ? c.take<G2J>(sh.gtmp_cap) : nullptr;
    utmp[0] = units && !sh.smsum ? c.take<G1J>(pl.unit_gsum.level_off[1] + 1) : nullptr;
    utmp[1] = units && !sh.smsum ? c.take<G1J>(pl.unit_gsum.level_off[1] + 1) : nullptr;
    b.set_flag = c.take<uint32_t>(n);
    b.flag_count = c.take<uint32_t>(1);
    b.f = c.take<Fp12>(sh.n_total);
    b.ml_lines = sigagg ? c.take<uint32_t>(mlq_line_words(sh.n_total)) : nullptr;
    if (sh.use_msm) {
      msm.off = c.take<uint32_t>(MSM_BUCKETS + 1);
      msm.seg_off = c.take<uint32_t>(MSM_BUCKETS + 1);
      msm.ent = c.take<uint32_t>(8ull * n);
      msm.sorted = c.take<uint32_t>(8ull * n);
      msm.seg_sum = c.take<G2J>(msm_seg_cap(n));
      msm.bucket = c.take<G2J>(MSM_BUCKETS);
      msm.win = c.take<G2J>(4);
    }
    b.req_status = c.take<int32_t>(R);
    g.f = gt ? c.take<Fp12>(R) : nullptr;
    g.fe = gt ? c.take<Fp12>(sh.grp_cap) : nullptr;
    b.chunk_fe = gt ? c.take<Fp12>(n_chunks) : nullptr;
    fe_save = sh.fe_simt_possible ? c.take<Fp12>(4ull * (n_chunks > R ? n_chunks : R)) : nullptr;
    if (sh.partial || sh.merged) {
      ptree[0] = c.take<Fp12>((sh.n_total + FPROD_FAN - 1) / FPROD_FAN);
      ptree[1] = c.take<Fp12>((sh.n_total + FPROD_FAN - 1) / FPROD_FAN);
    }
  }
  // results: written by the kernels straight into host-mapped memory
  void carve_res(Carver& c) {
    b.chunk_ok = c.take<int32_t>(sh.n_chunks);
    b.indiv_verdict = c.take<int32_t>(sh.R);
    g.verdict = c.take<int32_t>(sh.grp_cap);
    b.req_status_host = c.take<int32_t>(sh.R);
    b.flag_count_host = c.take<uint32_t>(1);
    merged_ok = sh.merged ? c.take<int32_t>(1) : nullptr;
  }

  // the fields of b that are no pointers into the carve
  void fill_fields() {
    b.first_bad_pk = b.pubkeys ? ctx->first_bad + ctx->first_bad_slot : nullptr;
    b.first_bad_pk_next = ctx->first_bad + (ctx->first_bad_slot ^ 1u);
    b.init_set_flag = sh.init_set_flag;
    b.n_sets = sh.n;
    b.n_reqs = sh.R;
    b.n_chunks = sh.n_chunks;
    if (a.pk) {
      b.pk_table = a.pk->table();
      b.pk_table_n = a.pk->snap.n;
      if (a.pk->comb() && !(ctx->debug_flags & BLS_DEBUG_NO_PK_COMB)) {
        b.pk_comb = a.pk->comb();
        b.pk_comb_ok = a.pk->comb_ok();
        b.pk_comb_n = a.pk->snap.comb_n;
      }
    }
    if (!(ctx->debug_flags & BLS_DEBUG_NO_PK_COMB)) b.g1_comb = (const Fp*)(*ctx->pkt)->g1_comb();
    b.scalar_base = a.scalar_base;
    b.pack = sh.pack;
    b.mlf_pl = sh.mlf_pl;
    b.multi_set_rules = sh.partial ? 1u : 0u;
    b.sigagg = sh.sigagg ? 1u : 0u;
    b.unit_base = sh.unit_base;
    b.n_units = sh.n_units;
    b.indiv_vbase = sh.indiv_vbase;
    b.n_agg = (uint32_t)pl.agg_list.size();
    b.agg_min = pl.agg_list.empty() ? 0u : BLS_AGG_WAVE_MIN;
    b.n_uniq = sh.dedup ? sh.n_uniq : 0;
    if (!bits_list.empty()) {
      b.cm_groups = ctx->cm_dev;
      b.n_bits = (uint32_t)bits_list.size();
    }
    if (!span_list.empty()) {
      b.cm_groups = ctx->cm_dev;
      b.n_span = (uint32_t)span_list.size();
    }
  }

  template <class T>
  void stage_vec(const T* dev_ptr, const std::vector<T>& v) {
    stage_copy(ctx, dev_ptr, v.data(), sizeof(T) * v.size());
  }

  void copy_plans() {
    if (sh.use_units) {
      stage_vec(b.set_unit, pl.units.set_unit);
      stage_vec(unit_rep_dev, pl.units.unit_rep);
      stage_vec(b.unit_off, pl.units.unit_off);
      if (!sh.smsum) {
        stage_vec(ugsets_dev, pl.units.members);
        stage_vec(useg_dev, pl.unit_gsum.seg);
      }
    }
    if (sh.ml_shared) stage_vec(b.ml_dom, pl.ml_dom);
    if (sh.sigagg) {
      stage_vec(gsets_dev, pl.chunk_gsum.gsets);
      stage_vec(gseg_dev, pl.chunk_gsum.seg);
      if (sh.use_total) stage_vec(tseg_dev, pl.total_gsum.seg);
    }
    stage_vec(b.chunk_off, plan.chunk_off);
    stage_vec(b.chunk_reqs, plan.chunk_reqs);
    if (!pl.agg_list.empty()) stage_vec(b.agg_sets, pl.agg_list);
    if (!bits_list.empty()) stage_vec(b.bits_sets, bits_list);
    if (!span_list.empty()) stage_vec(b.span_sets, span_list);
    if (sh.dedup) {
      stage_vec(b.msg_uniq, pl.msg_uniq);
      stage_vec(b.msg_rep, pl.msg_rep);
    }
  }

  void copy_inputs(const uint32_t seed_words[8]) {
    const uint32_t n = sh.n;
    stage_copy(ctx, b.req_off, in->req_set_offsets, sizeof(uint32_t) * (sh.R + 1));
    stage_copy(ctx, b.seed, seed_words, sizeof(uint32_t) * 8);
    if (b.pubkeys) stage_copy(ctx, b.pubkeys, in->pubkeys, 96ull * n);
    if (b.set_pk_off) {
      stage_copy(ctx, b.set_pk_off, in->set_pk_offsets, sizeof(uint32_t) * (n + 1));
      stage_copy(ctx, b.pk_idx, in->pk_indices, sizeof(uint32_t) * sh.n_pk_idx);
    }
    if (!bits_list.empty()) {
      stage_copy(ctx, b.set_committee, a.cs->set_committee, sizeof(uint32_t) * n);
      stage_copy(ctx, b.set_bits_off, a.cs->set_bits_off, sizeof(uint32_t) * (n + 1));
      stage_copy(ctx, b.bits, a.cs->bits, a.cs->set_bits_off[n]);
    }
    if (!span_list.empty()) {
      stage_copy(ctx, b.set_span_off, a.ss->set_span_off, sizeof(uint32_t) * (n + 1));
      stage_copy(ctx, b.span_refs, a.ss->span_refs, sizeof(uint32_t) * a.ss->set_span_off[n]);
      stage_copy(ctx, b.set_bits_off, a.ss->set_bits_off, sizeof(uint32_t) * (n + 1));
      stage_copy(ctx, b.bits, a.ss->bits, a.ss->set_bits_off[n]);
    }
    if (sh.dep) {
      stage_copy(ctx, dep.pubkeys48, a.dep->pubkeys48, 48ull * n);
      stage_copy(ctx, dep.wc, a.dep->withdrawal_credentials, 32ull * n);
      stage_copy(ctx, dep.amounts, a.dep->amounts, 8ull * n);
      stage_copy(ctx, dep.domain, a.dep->domain, 32);
    } else {
      stage_copy(ctx, b.msgs, in->messages, 32ull * n);
    }
    if (in->signature_lens) {
      // bytes past a short signature's length are never read (the set fails INVALID_SIZE)
      for (uint32_t i = 0; i < n; ++i) {
        uint32_t len = in->signature_lens[i] < 96 ? in->signature_lens[i] : 96;
        uint8_t* dst = ctx->host_stage + ((const uint8_t*)b.sigs - ctx->host_stage_dev) + 96ull * i;
        memset(dst, 0, 96);
        memcpy(dst, in->signatures + 96ull * i, len);
      }
      stage_copy(ctx, b.sig_lens, in->signature_lens, sizeof(uint32_t) * n);
    } else {
      stage_copy(ctx, b.sigs, in->signatures, 96ull * n);
    }
  }

  // a group-sum plan must fit the workspace every pass keeps for one (bls/plan.hpp gsum_fits)
  int check_gsum(const GsumPlan& p) {
    if (gsum_fits(p, sh.n, sh.R)) return 0;
    snprintf(ctx->err, sizeof(ctx->err), "group-sum plan exceeds its workspace");
    return -3;
  }

  // ---- stage: seed, workspace, plans and inputs into the staging area
  int stage_inputs() {
    if (sh.sigagg)
      if (const int rc = check_gsum(pl.chunk_gsum)) return rc;
    uint32_t seed_words[8];
    uint8_t seed[32];
    if (in->seed) {
      memcpy(seed, in->seed, 32);
    } else if (getrandom(seed, 32, 0) != 32) {
      snprintf(ctx->err, sizeof(ctx->err), "getrandom failed");
      return -3;
    }
    scalar_words_from_be32(seed, seed_words);
    {
      Carver c{nullptr, 0}, cr{nullptr, 0};
      carve(c);
      carve_res(cr);
      if (ensure_dev(ctx, c.off) || ensure_host(ctx, input_end) ||
          ensure_mapped(ctx, cr.off, &ctx->host_res, &ctx->host_res_dev, &ctx->host_res_cap))
        return -1;
    }
    Carver c{ctx->dev_ws, 0, ctx->host_stage_dev, input_end};
    carve(c);
    Carver cr{ctx->host_res_dev, 0};
    carve_res(cr);
    fill_fields();
    copy_plans();
    copy_inputs(seed_words);
    return 0;
  }

  // the levels of a G2 group-sum plan and k_vset for its groups -> virtual sets vbase + g
  int launch_gsum(const GsumPlan& p, const uint32_t* seg_dev, uint32_t vbase) {
    b.gsets = gsets_dev;
    const G2J* sums = nullptr;
    if (gsum_levels(ctx, b, p, seg_dev, gtmp, "k_gsum", &sums, s)) return -1;
    const size_t levels = p.level_off.size() - 1;
    const uint32_t G = levels ? p.level_off[levels] - p.level_off[levels - 1] : 0;
    HIPC(ctx, launch_k_vset(b, sums, G, vbase, s)); dbg_sync(s, "k_vset");
    return 0;
  }

  // ---- stage: the first pass.  stage_ms[1] k_pk, [2] k_pre, [3] k_chain (or k_pset), [4]
  // the signature sums (k_gsum / k_msm / k_smsum, units), [5] the Miller loops (k_mln; the
  // per-set path has none of its own): the per-kernel launch times bench.py prices
  int first_pass() {
    HIPC(ctx, hipEventRecord(ctx->ev0, s));
    HIPC(ctx, hipEventRecord(ctx->ev[0], s));  // no H2D stage: the kernels read the mapped inputs
    if (sh.n == 0) {
      for (int i = 1; i <= 5; ++i) HIPC(ctx, hipEventRecord(ctx->ev[i], s));
      return 0;
    }
    // either also resets set_flag, flag_count, the next first_bad_pk slot
    if (sh.dep) {
      HIPC(ctx, launch_k_deposit(b, dep, s)); dbg_sync(s, "k_deposit");
    } else {
      HIPC(ctx, launch_k_pk(b, s));
      HIPC(ctx, launch_k_pk_agg(b, s));
      HIPC(ctx, launch_k_pk_bits(b, s));
      HIPC(ctx, launch_k_pk_span(b, s)); dbg_sync(s, "k_pk");
    }
    ctx->first_bad_slot ^= 1u;
    HIPC(ctx, hipEventRecord(ctx->ev[1], s));
    HIPC(ctx, launch_k_pre(b, s)); dbg_sync(s, "k_pre");
    HIPC(ctx, hipEventRecord(ctx->ev[2], s));
    if (sh.sigagg) {
      if (first_pass_aggregated()) return -1;
    } else {
      HIPC(ctx, launch_k_pset(b, ctx->coop, s)); dbg_sync(s, "k_pset");
      HIPC(ctx, hipEventRecord(ctx->ev[3], s));
      HIPC(ctx, hipEventRecord(ctx->ev[4], s));
    }
    HIPC(ctx, hipEventRecord(ctx->ev[5], s));
    return 0;
  }

  // per-set chains, the chunks' sums of r sig -> virtual sets n + c, the units' sums, then
  // every Miller loop (sets and virtual sets) in one launch
  int first_pass_aggregated() {
    HIPC(ctx, launch_k_chain(b, s, sh.use_msm ? 0xBu : 0xFu)); dbg_sync(s, "k_chain");
    HIPC(ctx, hipEventRecord(ctx->ev[3], s));
    if (sh.smsum) {
      // each job's two pairing inputs in one step (kernels/k_smsg.hip)
      HIPC(ctx, launch_k_smsum(b, unit_rep_dev, s)); dbg_sync(s, "k_smsum");
    } else if (sh.use_msm) {
      msm.cnt = ctx->msm_state;
      msm.ticket = ctx->msm_state + MSM_BUCKETS;
      // the f-side shape (below) also decides the sum's form: the overlapped one rides on
      // k_mlf<1>'s launch
      choose_mlf_pl();
      msm_overlapped = sh.msm_overlap && k_mln_list_ok(b) && (b.mlf_pl == 1 || b.mlf_pl == 2 || b.mlf_pl == 4);
      if (msm_overlapped) {
        // the sort alone (it needs chain_live); the rest runs beside the Miller loops
        HIPC(ctx, launch_k_msm_sort(b, msm, s)); dbg_sync(s, "k_msm sort");
      } else {
        HIPC(ctx, launch_k_msm(b, msm, sh.n_chunks, sh.n, s)); dbg_sync(s, "k_msm");
      }
    } else if (sh.use_total ? launch_gsum(pl.total_gsum, tseg_dev, sh.n) : launch_gsum(pl.chunk_gsum, gseg_dev, sh.n)) {
      return -1;
    }
    if (sh.use_units && !sh.smsum) {
      // sum r_i pk_i per unit (levels over the members), then the units' chain entries
      b.gsets = ugsets_dev;
      const G1J* usums = nullptr;
      if (gsum_levels(ctx, b, pl.unit_gsum, useg_dev, utmp, "k_gsum1", &usums, s)) return -1;
      HIPC(ctx, launch_k_uset(b, usums, unit_rep_dev, s)); dbg_sync(s, "k_uset");
      b.gsets = gsets_dev;
    }
    HIPC(ctx, hipEventRecord(ctx->ev[4], s));
    choose_mlf_pl();
    if (msm_overlapped) {
      // sets and units with the sum's stages on the launches' lowest blocks; the virtual
      // sets exist when the f-side launch ends.  Only group 0's is live (the others are
      // written as infinity, f = 1, bls/msm.hpp msm_final_lane), so it alone is paired: one
      // cooperative wavefront, or the SIMT pair where there is no such program
      HIPC(ctx, launch_k_mlqf_msm(b, msm, sh.n_chunks, sh.n_units, b.ml_lines, s)); dbg_sync(s, "k_mlqf_msm");
      hipError_t e = launch_k_mln_coop(b, ctx->coop, sh.n, 1, nullptr, s);
      if (e == hipErrorNotSupported) {
        const uint32_t pl_pass = b.mlf_pl;  // (launch_ml_alone picks its own shape)
        e = launch_ml_alone(sh.n, 1, nullptr);
        b.mlf_pl = pl_pass;
      }
      HIPC(ctx, e); dbg_sync(s, "k_mln sum");
      return 0;
    }
    // a same-message call's first pass has two Miller loops per job (its unit and its
    // signature sum) and one per 1-set job: few items that never share f, so they run as
    // the cooperative single-pair loops, one wavefront each (launch_k_mln_coop: ~1 ms
    // where the SIMT pair takes ~7 ms), while they fit $BLS_COOP_ML_MAX
    hipError_t ml_rc = hipErrorNotSupported;
    if (sh.sm && k_mln_list_ok(b) && !sh.pl_forced) {
      std::vector<uint32_t> items(plan.nonbatch_reqs);
      for (uint32_t ch = 0; ch < sh.n_chunks; ++ch) items.push_back(sh.n + ch);
      for (uint32_t u = 0; u < sh.n_units; ++u) items.push_back(sh.unit_base + u);
      if (items.size() <= knobs().coop_ml_max) {
        stage_vec(own_sets_dev, items);
        ml_rc = launch_k_mln_coop(b, ctx->coop, 0, (uint32_t)items.size(), own_sets_dev, s);
      }
    }
    if (ml_rc == hipErrorNotSupported) ml_rc = launch_k_mln(b, ctx->coop, 0, sh.indiv_vbase, s);
    HIPC(ctx, ml_rc); dbg_sync(s, "k_mln");
    return 0;
  }

  // the f-side shape is chosen once per call (other contexts change the sets in flight
  // meanwhile): the first pass's Miller-loop launch and stats->pass_shape use it
  void choose_mlf_pl() {
    if (!b.mlf_pl && k_mln_list_ok(b)) b.mlf_pl = mlf_per_lane(knobs(), bls_sets_in_flight());
  }

  // Merged check: FE(prod of every f_i) == 1 with one final exponentiation (k_fprod
  // tree 1024 -> 16 -> 1), before any per-chunk one.
  int launch_merged() { return fprod_tree(ctx, b.f, sh.n_prod, ptree, merged_ok, nullptr, s); }

  // after a stream sync: the merged verdict and the statuses, from the mapped result area
  void read_merged() {
    merged_verdict = *res_host(ctx, merged_ok);
    memcpy(merged_status.data(), res_host(ctx, b.req_status_host), sizeof(int32_t) * sh.R);
  }

  // ---- stage: statuses and the merged check, then the pass's first wait.  stage_ms[6]
  int merged_check() {
    pass_pl = b.mlf_pl;
    HIPC(ctx, launch_k_status(b, s)); dbg_sync(s, "k_status");
    if (sh.merged && launch_merged()) return -1;
    HIPC(ctx, hipEventRecord(ctx->ev[6], s));
    HIPC(ctx, pass_wait(ctx, s));
    if (sh.merged) read_merged();
    if (sh.n > 0) flagged = *res_host(ctx, b.flag_count_host);
    return 0;
  }

  // ---- stage (rare): sets the cooperative kernel could not finish (exceptional additions,
  // infinity signatures, special SSWU inputs) -> exact path, then the status (the exact
  // path may find a signature outside G2) and the merged check again
  int flagged_redo() {
    if (!flagged) return 0;
    HIPC(ctx, launch_k_exact(b, s)); dbg_sync(s, "k_exact");
    HIPC(ctx, launch_k_status(b, s)); dbg_sync(s, "k_status");
    if (sh.merged && launch_merged()) return -1;
    HIPC(ctx, pass_wait(ctx, s));
    if (sh.merged) read_merged();
    return 0;
  }

  // the per-set RS the fallback sums need: made by the first pass unless the MSM replaced
  // role 2 there
  int ensure_rs() {
    if (!rs_done) {
      HIPC(ctx, launch_k_chain(b, s, 0x4u)); dbg_sync(s, "k_chain rs");
      rs_done = true;
    }
    return 0;
  }
  // the Miller-loop launches after the first pass take their own items-per-lane
  // (mlf_per_lane_alone: their items never share f) unless a test forces one
  void alone_pl(uint32_t count) {
    const uint32_t pl_alone = mlf_per_lane_alone(knobs(), count);
    if (pl_alone && !sh.pl_forced && k_mln_list_ok(b)) b.mlf_pl = pl_alone;
  }
  // ... and up to $BLS_COOP_ML_MAX items they are cooperative single-pair loops, one
  // wavefront per item (launch_k_mln_coop), else the SIMT pair at that shape
  hipError_t launch_ml_alone(uint32_t first, uint32_t count, const uint32_t* items) {
    if (count == 0) return hipSuccess;
    if (!sh.pl_forced && k_mln_list_ok(b)) {
      const hipError_t e = launch_k_mln_coop(b, ctx->coop, first, count, items, s);
      if (e != hipErrorNotSupported) return e;
    }
    alone_pl(count);
    return items ? launch_k_mln_list(b, items, count, s) : launch_k_mln(b, ctx->coop, first, count, s);
  }

  // ---- stage: the chunk verdicts -- all 1 after a passing merged check, else (not in
  // partial mode) the per-chunk final exponentiations -- and the stats of the pass so far
  int chunk_checks() {
    const uint32_t n_chunks = sh.n_chunks;
    merged_pass = sh.merged && merged_verdict == 1;
    for (uint32_t r = 0; merged_pass && r < sh.R; ++r) merged_pass = merged_status[r] == BLS_OK;
    if (sh.merged && !sh.sm && !sh.dep) ctx->last_merged_failed = !merged_pass;
    if (merged_pass) {
      for (uint32_t ch = 0; ch < n_chunks; ++ch) chunk_ok[ch] = 1;
    } else if (n_chunks > 0 && !sh.partial) {
      // some set is invalid or erroneous (or no merged check): the per-chunk verdicts decide
      if (ensure_rs()) return -1;
      if (sh.use_total) {
        // the chunks' own signature sums and their Miller loops (virtual sets n + c)
        if (launch_gsum(pl.chunk_gsum, gseg_dev, sh.n)) return -1;
        HIPC(ctx, launch_ml_alone(sh.n, n_chunks, nullptr)); dbg_sync(s, "k_mln chunk sums");
      }
      // many chunk checks: one lane each (a failing pass at the plateau has hundreds, and a
      // cooperative task holds a SIMD for a whole final exponentiation); few: one wavefront
      // each, the shorter latency
      if (fe_save && n_chunks >= sh.fe_min) HIPC(ctx, launch_k_chunk_simt(b, fe_save, s));
      else {
        HIPC(ctx, launch_k_chunk_coop(b, ctx->coop, s));
        chunk_fe_kept = b.chunk_fe != nullptr;  // the checked chunks' final exponentiations
      }
      dbg_sync(s, "k_chunk");
      HIPC(ctx, pass_wait(ctx, s));
      memcpy(chunk_ok.data(), res_host(ctx, b.chunk_ok), sizeof(int32_t) * n_chunks);
    }
    if (sh.merged_skipped) {
      // the context keeps skipping the merged check while its passes keep failing a chunk
      bool all_ok = true;
      for (uint32_t ch = 0; ch < n_chunks; ++ch) all_ok = all_ok && chunk_ok[ch] == 1;
      ctx->last_merged_failed = !all_ok;
    }
    if (a.stats) {
      a.stats->merged_check = sh.merged ? (merged_pass ? 1 : 2) : (sh.merged_skipped ? 3 : 0);
      a.stats->pass_shape = sh.sigagg ? ((sh.use_msm ? 1u : 0u) | (msm_overlapped ? 2u : 0u) |
                                         (k_mln_list_ok(b) ? pass_pl << 8 : 0u))
                                      : 0u;
      a.stats->n_flagged = flagged;
      a.stats->n_unique_msgs = sh.n_uniq;
      a.stats->n_ml_units = sh.n_units;
    }
    return 0;
  }

  // ---- stage (partial mode, instead of the ones below): the shard's status and the
  // product of its f.
  // The call rejects with the code of its first error, classes in the reference's
  // order: a pubkey that does not decode / aggregate (deserializeSet and
  // getAggregatedPubkey run before anything else, worker.ts:45, index.ts:160), then a
  // signature that does not decode (maybeBatch.ts:19-24 maps fromBytes over the
  // sets), then an infinity pubkey (verifyMultipleSignatures).  The shard reports its
  // first error of the lowest class with its set index, so the ranks can reduce
  // (class, call index) in that order (lodestar_amd/shard.py).
  int partial_result() {
    const uint32_t n = sh.n, R = sh.R;
    std::vector<int32_t> st(res_host(ctx, b.req_status_host), res_host(ctx, b.req_status_host) + R);
    *a.partial_status = 0;
    for (uint32_t r = 0; r < R && !*a.partial_status; ++r)
      if (st[r] != 0) *a.partial_status = -st[r];
    if (*a.partial_status && n > 0) {
      std::vector<int32_t> pks(n), sgs(n);
      std::vector<uint8_t> inf(n);
      HIPC(ctx, hipMemcpyAsync(pks.data(), b.pk_status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
      HIPC(ctx, hipMemcpyAsync(sgs.data(), b.sig_status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
      HIPC(ctx, hipMemcpyAsync(inf.data(), b.pk_inf, n, hipMemcpyDeviceToHost, s));
      HIPC(ctx, pass_wait(ctx, s));
      uint32_t cls = 3, idx = 0;
      int32_t code = 0;
      for (uint32_t i = 0; i < n && cls > 0; ++i)
        if (pks[i] != BLS_OK) { cls = 0; idx = i; code = pks[i]; }
      for (uint32_t i = 0; i < n && cls > 1; ++i)
        if (sgs[i] != BLS_OK) { cls = 1; idx = i; code = sgs[i]; }
      for (uint32_t i = 0; i < n && cls > 2; ++i)
        if (inf[i]) { cls = 2; idx = i; code = BLS_PK_IS_INFINITY; }
      if (cls < 3) *a.partial_status = -code;  // else: an empty-request code (kept)
      if (a.partial_err) {
        a.partial_err[0] = cls;
        a.partial_err[1] = idx;
      }
    }
    if (*a.partial_status || n == 0) return 0;
    const Fp12* prod = nullptr;
    if (fprod_tree(ctx, b.f, sh.n_prod, ptree, nullptr, &prod, s)) return -1;
    HIPC(ctx, hipMemcpyAsync(a.partial_out, prod, sizeof(Fp12), hipMemcpyDeviceToHost, s));
    HIPC(ctx, pass_wait(ctx, s));
    if (a.stats) {
      float ms = 0.f;
      HIPC(ctx, hipEventRecord(ctx->ev1, s));
      HIPC(ctx, hipEventSynchronize(ctx->ev1));
      (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
      a.stats->device_ms = ms;
    }
    return 0;
  }

  // Aggregated path: each individually verified request pairs the sum of its own r sig
  // (virtual sets indiv_vbase + t), and a request whose sets were paired in their chunk's
  // units or shared loops (its chunk failed) now runs their own Miller loops.
  int indiv_miller_loops() {
    const uint32_t* req_off = in->req_set_offsets;
    const size_t first_t = plan.nonbatch_reqs.size();
    const bool shared = sh.use_units || sh.ml_shared;
    const bool own_list = shared && k_mln_list_ok(b);
    // a set needs its own Miller loop again only when the first pass did not leave it
    // one: it was paired in its chunk's unit (f_i = 1), or its f was shared with the
    // next items of its lane (more than one item per k_mlf lane); at one item per lane
    // or per lane pair f_i = e(r_i pk_i, H(m_i)) already
    const bool f_shared = sh.ml_shared && !(pass_pl == 1u || pass_pl == MLF_PAIR);
    std::vector<uint32_t> own;
    if (own_list) {
      // every such set of the failed chunks' requests, in ONE launch with the requests'
      // signature sums below (one Miller-loop latency instead of two on the failing
      // call's path, profiles/r05_cfg5_fallback.json)
      plan_own_sets(req_off, iv.reqs, first_t, f_shared, sh.use_units ? pl.units.set_unit.data() : nullptr, own);
    } else if (shared) {
      std::vector<uint32_t> runs;
      plan_own_runs(req_off, iv.reqs, first_t, runs);
      for (size_t k = 0; k < runs.size(); k += 2) {
        alone_pl(runs[k + 1]);
        HIPC(ctx, launch_k_mln(b, ctx->coop, runs[k], runs[k + 1], s, true)); dbg_sync(s, "k_mln own");
      }
    }
    std::vector<uint32_t> goff(n_sum + 1);
    for (size_t t = 0; t <= n_sum; ++t) goff[t] = (uint32_t)t;
    plan_gsum(req_off, goff, iv.reqs, indiv_gsum);  // (the groups are the first n_sum requests)
    if (ensure_rs()) return -1;
    if (const int rc = check_gsum(indiv_gsum)) return rc;
    if (n_sum > 0) {  // (under group sums every request may be group-tested)
      stage_vec(gsets_dev, indiv_gsum.gsets);
      stage_vec(gseg_dev, indiv_gsum.seg);
      if (launch_gsum(indiv_gsum, gseg_dev, sh.indiv_vbase)) return -1;
    }
    if (own_list) {
      for (size_t t = 0; t < n_sum; ++t) own.push_back(sh.indiv_vbase + (uint32_t)t);
      if (!own.empty()) {
        stage_vec(own_sets_dev, own);
        HIPC(ctx, launch_ml_alone(0, (uint32_t)own.size(), own_sets_dev));
        dbg_sync(s, "k_mln own + indiv (list)");
      }
    } else {
      HIPC(ctx, launch_ml_alone(sh.indiv_vbase, n_sum, nullptr)); dbg_sync(s, "k_mln indiv");
    }
    return 0;
  }

  // each request's product: groups of BLS_FOLD consecutive sets multiplied in parallel
  // first (as groups of BLS_FOLD1, then those partial products BLS_FOLD / BLS_FOLD1 at a
  // time), then one final exponentiation per directly verified request
  int indiv_products() {
    plan_fold_groups(in->req_set_offsets, iv.reqs, fold);
    b.fold = 1;
    b.n_fold = 0;
    if (fold.any_fold) {
      b.fold = BLS_FOLD;
      b.n_fold = (uint32_t)(fold.groups.size() / 2);
      stage_vec(b.fold_groups, fold.groups);
      HIPC(ctx, launch_k_fold(b, ctx->coop, b.fold_groups, fold.n_fold1, 1, s)); dbg_sync(s, "k_fold");
      HIPC(ctx, launch_k_fold(b, ctx->coop, b.fold_groups + 2ull * fold.n_fold1, b.n_fold - fold.n_fold1, BLS_FOLD1, s));
      dbg_sync(s, "k_fold2");
    }
    g.n_direct = iv.n_direct;
    g.sum_f = gsums ? b.f + sh.indiv_vbase + iv.n_direct : nullptr;
    if (fe_save && b.n_indiv >= sh.fe_min) HIPC(ctx, launch_k_indiv_simt(b, g, fe_save, s));
    else HIPC(ctx, launch_k_indiv_coop(b, ctx->coop, g, s));
    dbg_sync(s, "k_indiv");
    return 0;
  }

  // ---- stage: the requests verified on their own (bls/plan.hpp plan_indiv).  stage_ms[7]
  // (with the group tests)
  int individual_pass() {
    plan_indiv(plan, chunk_ok.data(), sh.gt_min, iv);
    // Group sums: on the aggregated path, with many requests group-tested, a group-tested
    // request pairs no signature sum of its own; each group test pairs ONE sum over its
    // requests' sets (group_sums) -- 4-6 Miller loops per failed chunk of 16 instead of 16
    // (group_sums_min).
    gsums = sh.sigagg && !iv.gt_chunks.empty() && iv.reqs.size() - iv.n_direct >= sh.gsums_min;
    n_sum = gsums ? iv.n_direct : (uint32_t)iv.reqs.size();
    indiv_verdict.assign(iv.reqs.size() + 1, 0);
    if (!iv.reqs.empty()) {
      b.n_indiv = (uint32_t)iv.reqs.size();
      stage_vec(b.indiv_reqs, iv.reqs);  // the stream is idle
      HIPC(ctx, hipEventRecord(ctx->ev[7], s));
      if (sh.sigagg)
        if (const int rc = indiv_miller_loops()) return rc;
      if (indiv_products()) return -1;
      if (iv.gt_chunks.empty()) HIPC(ctx, hipEventRecord(ctx->ev[8], s));
    }
    if (iv.gt_chunks.empty()) HIPC(ctx, hipEventRecord(ctx->ev1, s));
    HIPC(ctx, pass_wait(ctx, s));
    if (!iv.reqs.empty())
      memcpy(indiv_verdict.data(), res_host(ctx, b.indiv_verdict), sizeof(int32_t) * iv.reqs.size());
    return 0;
  }

  // Group sums (aggregated path): the tests' own signature sums, sum of r_i sig_i over
  // their requests' sets, paired ML(-g1, .) before k_group_coop.  Test g's sum lands in
  // virtual set indiv_vbase + n_direct + g (the group-tested requests' own slots, unused
  // under group sums; a pass never has more tests than group-tested requests).  Returns 0,
  // 1 when the plan does not fit the workspace (nothing ran: group_rounds_ab), < 0 on an
  // error.
  int group_sums(const std::vector<uint32_t>& goff, const std::vector<uint32_t>& gmem) {
    const uint32_t T = (uint32_t)(goff.size() - 1);
    if (iv.n_direct + T > iv.reqs.size()) return 1;
    std::vector<uint32_t> reqs(gmem.size());
    for (size_t k = 0; k < gmem.size(); ++k) reqs[k] = iv.reqs[gmem[k]];
    GsumPlan gp;
    plan_gsum(in->req_set_offsets, goff, reqs, gp);
    if (!gsum_fits(gp, sh.n, sh.R)) return 1;
    stage_vec(gsets_dev, gp.gsets);  // the stream is idle
    stage_vec(gseg_dev, gp.seg);
    if (launch_gsum(gp, gseg_dev, sh.indiv_vbase + iv.n_direct)) return -1;
    HIPC(ctx, launch_ml_alone(sh.indiv_vbase + iv.n_direct, T, nullptr)); dbg_sync(s, "k_mln group sums");
    return 0;
  }

  // run the tests (goff: offsets into gmem, indices into the indiv list); results in gv
  // (bit 0: passed; bit 1, with ref: its final exponentiation equals test ref[g]'s);
  // 1 when the group sums do not fit (nothing ran)
  int run_group_tests(const std::vector<uint32_t>& goff, const std::vector<uint32_t>& gmem, std::vector<int32_t>& gv,
                      const std::vector<uint32_t>* ref = nullptr) {
    gv.assign(goff.size() - 1, 0);
    if (gv.empty()) return 0;
    if (gsums)
      if (const int rc = group_sums(goff, gmem)) return rc;
    stage_vec(g.off, goff);  // the stream is idle
    stage_vec(g.members, gmem);
    g.n = (uint32_t)gv.size();
    GroupBufs gg = g;
    if (ref) stage_vec(g.ref, *ref);
    else gg.fe = nullptr;
    HIPC(ctx, launch_k_group_coop(b, ctx->coop, gg, s)); dbg_sync(s, "k_group_coop");
    HIPC(ctx, pass_wait(ctx, s));
    memcpy(gv.data(), res_host(ctx, g.verdict), sizeof(int32_t) * gv.size());
    return 0;
  }

  int group_rounds_ab(const std::vector<GtChunk>& chunks, bool eq, std::vector<uint32_t>& alone);
  int verify_groups();

  // ---- stage: group tests over the failed chunks large enough for them
  int group_tests() {
    if (iv.gt_chunks.empty()) return 0;
    g.ref_fe = chunk_fe_kept ? b.chunk_fe : nullptr;
    if (const int rc = verify_groups()) return rc;
    HIPC(ctx, hipEventRecord(ctx->ev[8], s));
    HIPC(ctx, hipEventRecord(ctx->ev1, s));
    HIPC(ctx, pass_wait(ctx, s));
    return 0;
  }

  // ---- stage: verdicts and stats.  stage_ms[k], k = 1 .. 6: from event k - 1 to event k
  // ([0]: no H2D stage, ~0; [1] k_pk, [2] k_pre, [3] k_chain or k_pset, [4] the sums, [5] the
  // Miller loops, [6] k_status + the merged check); [7]: the individual pass with its group
  // tests (0 without one).  A flagged redo and the chunk checks fall between [6] and [7]:
  // in device_ms only.
  void finish() {
    assemble_verdicts(in, plan, chunk_ok.data(), iv.reqs, indiv_verdict.data(), a.verdicts, a.stats);
    if (!a.stats) return;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    a.stats->device_ms = ms;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev[0]);
    a.stats->stage_ms[0] = ms;
    for (int i = 1; i <= 6; ++i) {
      (void)hipEventElapsedTime(&ms, ctx->ev[i - 1], ctx->ev[i]);
      a.stats->stage_ms[i] = ms;
    }
    a.stats->stage_ms[7] = 0.0;
    if (!iv.reqs.empty()) {
      (void)hipEventElapsedTime(&ms, ctx->ev[7], ctx->ev[8]);
      a.stats->stage_ms[7] = ms;
    }
  }
};

// Group tests of the failed chunks iv.gt_chunks (the comment above group_test_min, bls/knobs.hpp): pass A
// (bls/plan.hpp plan_group_tests_a), its decode (bls/group_decode.hpp, or pass B without
// complement inference), pass C for what is left; verdicts into indiv_verdict.
//
// Passes A and B over `chunks`; the requests left for pass C are appended to `alone`.
// Returns 0, < 0 on an error, or 1 when pass A's group sums do not fit the workspace and
// nothing ran: a bit group holds half its chunk's requests, so pass A sums ~nbits / 2 times
// the chunk's sets, and the sum workspace holds the pass's n sets once -- a pass most of
// whose sets sit in failed chunks does not fit in one round (the caller splits the chunks).
// A single chunk that does not fit goes to pass C.
int VerifyPass::group_rounds_ab(const std::vector<GtChunk>& chunks, bool eq, std::vector<uint32_t>& alone) {
  std::vector<int32_t>& verdict = indiv_verdict;
  uint32_t* cnt = ctx->gt_counts;  // (bls_gpu_group_test_counts)
  GroupTestsA pa;
  plan_group_tests_a(chunks, verdict.data(), eq, sh.gt_eq_mode != 2 && g.ref_fe, pa);
  std::vector<GroupTestChunk>& cs = pa.cs;
  if (!group_tests_fit(pa, sh.R, sh.n_chunks)) {
    snprintf(ctx->err, sizeof(ctx->err), "group-test plan exceeds its workspace");
    return -3;
  }
  std::vector<int32_t> gv;
  std::vector<uint32_t> goff_b{0}, gmem_b;
  std::vector<size_t> in_b;
  const int rc_a = run_group_tests(pa.off, pa.members, gv, eq ? &pa.ref : nullptr);
  if (rc_a < 0) return -1;
  if (rc_a == 1 && chunks.size() > 1) return 1;
  cnt[0] += (uint32_t)cs.size();
  for (const GroupTestChunk& c : cs) cnt[1] += eq && !c.whole ? 1u : 0u;  // (ref = REF_CHUNK | chunk)
  if (rc_a == 1) {  // the group sums of one chunk's pass A do not fit: its requests alone
    cnt[7] = 1;
    for (const GroupTestChunk& c : cs) alone.insert(alone.end(), c.ok.begin(), c.ok.end());
    return 0;
  }
  cnt[2] += (uint32_t)gv.size();
  // complement inference: with the test of all the chunk's requests (A) beside each bit
  // group G_j, FE(G_j) FE(rest_j) = FE(A) decides the complement too (FE(rest_j) == 1 iff
  // FE(G_j) == FE(A)), so a single invalid request b shows as exactly one failing test per
  // bit -- G_j where b's bit j is set, rest_j where it is clear -- and every other request
  // sits in a passing test: no pass B.  Both G_j and rest_j failing (two or more invalid)
  // or an index past m: pass C.
  for (size_t i = 0; eq && i < cs.size(); ++i) {
    const GroupTestChunk& c = cs[i];
    const uint32_t m = (uint32_t)c.ok.size();
    // without a whole test the whole is the failed chunk check (it failed)
    const bool pass = c.whole && (gv[c.first] & 1) != 0;
    const int32_t bad = group_decode(m, c.nbits, pass, gv.data() + c.first + (c.whole ? 1u : 0u));
    if (bad < 0) {
      alone.insert(alone.end(), c.ok.begin(), c.ok.end());
      continue;
    }
    for (uint32_t k = 0; k < m; ++k) verdict[c.ok[k]] = (int32_t)k == bad ? 0 : 1;
    ++cnt[3];
  }
  if (eq) cs.clear();
  // decode pass A; plan pass B
  for (size_t i = 0; i < cs.size(); ++i) {
    GroupTestChunk& c = cs[i];
    uint32_t idx = c.first;
    const uint32_t m = (uint32_t)c.ok.size();
    if (c.has_err || m == 1) {
      const bool pass = gv[idx++] == 1;
      if (pass || m == 1) {
        for (uint32_t t : c.ok) verdict[t] = pass ? 1 : 0;
        ++cnt[3];
        continue;
      }
    }
    uint32_t bad = 0;
    for (uint32_t j = 0; j < c.nbits; ++j)
      if (gv[idx + j] != 1) bad |= 1u << j;
    if (bad >= m) {
      alone.insert(alone.end(), c.ok.begin(), c.ok.end());
      continue;
    }
    c.b = (int32_t)bad;
    gmem_b.push_back(c.ok[bad]);
    goff_b.push_back((uint32_t)gmem_b.size());
    for (uint32_t k = 0; k < m; ++k)
      if (k != bad) gmem_b.push_back(c.ok[k]);
    goff_b.push_back((uint32_t)gmem_b.size());
    in_b.push_back(i);
  }
  const int rc_b = in_b.empty() ? 0 : run_group_tests(goff_b, gmem_b, gv);
  if (rc_b < 0) return -1;
  if (!in_b.empty() && rc_b == 0) cnt[4] += (uint32_t)gv.size();
  for (size_t q = 0; q < in_b.size(); ++q) {
    GroupTestChunk& c = cs[in_b[q]];
    if (rc_b == 0 && gv[2 * q] == 0 && gv[2 * q + 1] == 1) {
      for (uint32_t k = 0; k < c.ok.size(); ++k) verdict[c.ok[k]] = (int32_t)k == c.b ? 0 : 1;
      ++cnt[5];
    } else {
      alone.insert(alone.end(), c.ok.begin(), c.ok.end());
    }
  }
  return 0;
}

int VerifyPass::verify_groups() {
  std::vector<int32_t>& verdict = indiv_verdict;
  const bool eq = sh.gt_eq_mode != 0 && g.fe;
  std::vector<uint32_t> alone;  // requests for pass C
  // passes A and B: every chunk in one round when its group sums fit (they do unless most
  // of the pass failed), else the chunk list in halves until they do
  std::vector<std::pair<size_t, size_t>> todo{{0, iv.gt_chunks.size()}};
  while (!todo.empty()) {
    const std::pair<size_t, size_t> part = todo.back();
    todo.pop_back();
    const std::vector<GtChunk> chunks(iv.gt_chunks.begin() + part.first, iv.gt_chunks.begin() + part.second);
    const int rc = group_rounds_ab(chunks, eq, alone);
    if (rc < 0) return rc;
    if (rc == 1) {
      const size_t mid = part.first + (part.second - part.first) / 2;
      todo.push_back({mid, part.second});
      todo.push_back({part.first, mid});
    }
  }
  // pass C: one test per request
  std::vector<int32_t> gv;
  std::vector<uint32_t> goff_c{0};
  for (size_t k = 0; k < alone.size(); ++k) goff_c.push_back((uint32_t)k + 1);
  const int rc_c = run_group_tests(goff_c, alone, gv);
  if (rc_c != 0) {
    // one request per test always fits the request-sum workspace
    snprintf(ctx->err, sizeof(ctx->err), "group tests: per-request sums do not fit");
    return -3;
  }
  ctx->gt_counts[6] = (uint32_t)alone.size();
  for (size_t k = 0; k < alone.size(); ++k) verdict[alone[k]] = gv[k] == 1 ? 1 : 0;
  return 0;
}

int verify_body(bls_gpu_ctx* ctx, const bls_batch* in, const PassArgs& a) {
  memset(ctx->gt_counts, 0, sizeof(ctx->gt_counts));
  HIPC(ctx, hipSetDevice(ctx->device));
  if (a.stats) memset(a.stats, 0, sizeof(*a.stats));
  if (in->n_reqs == 0) return 0;
  // (a deposit call built its batch itself, with neither keys nor messages on the host)
  if (!a.dep)
    if (const int rc = check_batch(in, "batch", ctx->err, sizeof(ctx->err))) return rc;
  const InFlight in_flight(in->n_sets);
  VerifyPass p(ctx, in, a);
  int rc;
  if ((rc = p.stage_inputs())) return rc;
  if ((rc = p.first_pass())) return rc;
  if ((rc = p.merged_check())) return rc;
  if ((rc = p.flagged_redo())) return rc;
  if ((rc = p.chunk_checks())) return rc;
  if (p.sh.partial) return p.partial_result();
  if ((rc = p.individual_pass())) return rc;
  if ((rc = p.group_tests())) return rc;
  p.finish();
  return 0;
}

}  // namespace

// One call under the context's lock.  A call that fails part-way may leave the MSM's
// bucket counters / tickets (reset only by the kernels' last workgroups) mid-pass: they
// are zeroed again before the context takes another call.
// `a`: zero but for the entry point's own fields; a.pk is filled here.
static int verify_impl(bls_gpu_ctx* ctx, const bls_batch* in, PassArgs a) {
  CTX_LOCK(ctx);
  ctx->wait_block = wait_blocks(knobs(), in->n_sets);
  // the table as this call sees it: kept until the stream is idle (every stage of a pass
  // that ran to its end has waited; one that failed part-way is waited for below), so a
  // load through another context never frees a buffer under this call's kernels
  PkView pk;
  if (!a.dep) pk = pk_snapshot(ctx);
  a.pk = a.dep ? nullptr : &pk;
  const int rc = verify_body(ctx, in, a);
  if (rc != 0) (void)hipStreamSynchronize(ctx->stream);
  if (rc < 0 && ctx->msm_state) {
    (void)hipMemsetAsync(ctx->msm_state, 0, sizeof(uint32_t) * MSM_STATE_WORDS, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
  }
  return rc;
}

// The aggregate key of each of n_sets sets, as the three bls_gpu_aggregate_* calls return it.
// The entry point's `inputs` carves the arrays it stages into b; its `front` copies them in
// and launches its front kernel (the sets' sums into b.pk).  The vectors those copies read
// are the entry point's, so they outlive the call's OneShot.  k_aggregate then serializes
// every set (stage_pk skips the ones a front kernel summed).
template <class Inputs, class Front>
static int aggregate_sets(bls_gpu_ctx* ctx, uint32_t n_sets, uint8_t* out96, int32_t* codes, Inputs&& inputs,
                          Front&& front) {
  PipeBufs b;
  memset(&b, 0, sizeof(b));
  const PkView pk = pk_snapshot(ctx);  // dropped at return, after the stream's tail (run)
  uint8_t* d_out = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) {
        inputs(c, b);
        c.buf(b.pk, n_sets).buf(b.pk_status, n_sets).buf(d_out, 96ull * n_sets);
      }))
    return -1;
  b.n_sets = n_sets;
  b.pk_table = pk.table();
  b.pk_table_n = pk.snap.n;
  if (const int rc = front(b, run.s)) return rc;
  HIPC(ctx, launch_k_aggregate(b, d_out, run.s));
  HIPC(ctx, hipMemcpyAsync(out96, d_out, 96ull * n_sets, hipMemcpyDeviceToHost, run.s));
  if (codes) HIPC(ctx, hipMemcpyAsync(codes, b.pk_status, sizeof(int32_t) * n_sets, hipMemcpyDeviceToHost, run.s));
  return run.finish();
}

extern "C" {

int bls_gpu_verify(bls_gpu_ctx* ctx, const bls_batch* in, int32_t* verdicts, bls_stats* stats) {
  return verify_impl(ctx, in, PassArgs{verdicts, stats});
}

int bls_gpu_verify_committees(bls_gpu_ctx* ctx, const bls_batch* in, const bls_committee_sets* cs, int32_t* verdicts,
                              bls_stats* stats) {
  if (!ctx || !in) return -2;
  {
    CTX_LOCK(ctx);  // (for ctx->err; verify_impl takes the lock for the call itself)
    if (in->n_sets && !in->set_pk_offsets) {
      snprintf(ctx->err, sizeof(ctx->err), "committee sets: the batch must carry table indices (set_pk_offsets)");
      return -2;
    }
    if (const int rc = committee_check_sets(cs, in->n_sets, in->set_pk_offsets, ctx->err, sizeof(ctx->err))) return rc;
  }
  PassArgs a{verdicts, stats};
  a.cs = cs;
  return verify_impl(ctx, in, a);
}

int bls_gpu_verify_spans(bls_gpu_ctx* ctx, const bls_batch* in, const bls_span_sets* ss, int32_t* verdicts,
                         bls_stats* stats) {
  if (!ctx || !in) return -2;
  {
    CTX_LOCK(ctx);  // (for ctx->err; verify_impl takes the lock for the call itself)
    if (const int rc = span_check_sets(ss, in->n_sets, true, in->set_pk_offsets, ctx->err, sizeof(ctx->err))) return rc;
  }
  PassArgs a{verdicts, stats};
  a.ss = ss;
  return verify_impl(ctx, in, a);
}

int bls_gpu_verify_many(bls_gpu_ctx* ctx, const bls_batch* batches, uint32_t n_batches, int32_t* verdicts,
                        bls_stats* stats) {
  if (!ctx || (n_batches && (!batches || !verdicts))) return -2;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (n_batches == 0) return 0;
  if (n_batches == 1) return verify_impl(ctx, batches, PassArgs{verdicts, stats});
  // messages with raw pubkeys keep their own pass: deserializeSet rejects a whole
  // message (worker.ts:43-46), which the merged pass does not track per message
  bool merge = true;
  for (uint32_t k = 0; k < n_batches; ++k) merge = merge && batches[k].set_pk_offsets != nullptr;
  if (!merge) {
    uint32_t off = 0;
    for (uint32_t k = 0; k < n_batches; ++k) {
      bls_stats st;
      const int rc = verify_impl(ctx, &batches[k], PassArgs{verdicts + off, stats ? &st : nullptr});
      if (rc != 0) return rc;
      off += batches[k].n_reqs;
      if (stats) {
        stats->batch_retries += st.batch_retries;
        stats->batch_sigs_success += st.batch_sigs_success;
        stats->n_chunks += st.n_chunks;
        stats->n_individual += st.n_individual;
        stats->n_flagged += st.n_flagged;
        stats->n_unique_msgs += st.n_unique_msgs;
        stats->n_ml_units += st.n_ml_units;
        stats->pass_shape |= st.pass_shape;
        stats->device_ms += st.device_ms;
      }
    }
    return 0;
  }
  // one pass over the concatenated messages (SoA arrays joined, offsets rebased); each
  // message passes verify_impl's shape checks before anything is read through it
  uint32_t n = 0, R = 0, n_idx = 0;
  bool lens = false;
  for (uint32_t k = 0; k < n_batches; ++k) {
    const bls_batch& b = batches[k];
    char what[32];
    snprintf(what, sizeof(what), "batch %u", k);
    if (const int rc = check_batch(&b, what, ctx->err, sizeof(ctx->err))) return rc;
    if (b.n_reqs == 0 && b.n_sets != 0) {
      snprintf(ctx->err, sizeof(ctx->err), "%s: sets without requests", what);
      return -2;
    }
    n += b.n_sets;
    R += b.n_reqs;
    n_idx += b.set_pk_offsets[b.n_sets];
    lens = lens || b.signature_lens != nullptr;
  }
  std::vector<uint32_t> req_off(R + 1, 0), set_pk_off(n + 1, 0), pk_idx(n_idx ? n_idx : 1), sig_lens(lens ? n : 0);
  std::vector<uint8_t> batchable(R ? R : 1), msgs(32ull * n), sigs(96ull * n);
  std::vector<uint32_t> req_bounds(1, 0);
  uint32_t so = 0, ro = 0, io = 0;
  for (uint32_t k = 0; k < n_batches; ++k) {
    const bls_batch& b = batches[k];
    for (uint32_t r = 0; r < b.n_reqs; ++r) {
      req_off[ro + r + 1] = so + b.req_set_offsets[r + 1];
      batchable[ro + r] = b.req_batchable ? b.req_batchable[r] : 0;
    }
    for (uint32_t i = 0; i < b.n_sets; ++i) set_pk_off[so + i + 1] = io + b.set_pk_offsets[i + 1];
    if (b.set_pk_offsets[b.n_sets]) memcpy(&pk_idx[io], b.pk_indices, sizeof(uint32_t) * b.set_pk_offsets[b.n_sets]);
    if (b.n_sets) {
      memcpy(&msgs[32ull * so], b.messages, 32ull * b.n_sets);
      memcpy(&sigs[96ull * so], b.signatures, 96ull * b.n_sets);
    }
    for (uint32_t i = 0; lens && i < b.n_sets; ++i) sig_lens[so + i] = b.signature_lens ? b.signature_lens[i] : 96u;
    so += b.n_sets;
    ro += b.n_reqs;
    io += b.set_pk_offsets[b.n_sets];
    req_bounds.push_back(ro);
  }
  bls_batch all;
  memset(&all, 0, sizeof(all));
  all.n_sets = n;
  all.n_reqs = R;
  all.req_set_offsets = req_off.data();
  all.req_batchable = batchable.data();
  all.set_pk_offsets = set_pk_off.data();
  all.pk_indices = pk_idx.data();
  all.messages = msgs.data();
  all.signatures = sigs.data();
  all.signature_lens = lens ? sig_lens.data() : nullptr;
  all.seed = batches[0].seed;  // scalars: one random batch per pass (verdicts do not depend on them)
  PassArgs a{verdicts, stats};
  a.req_bounds = &req_bounds;
  return verify_impl(ctx, &all, a);
}

int bls_gpu_verify_same_message(bls_gpu_ctx* ctx, const bls_same_msg_batch* in, int32_t* set_verdicts,
                                bls_stats* stats) {
  if (!ctx || !in) return -2;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (in->n_jobs == 0) return 0;
  const uint32_t n = in->n_sets, J = in->n_jobs;
  auto bad = [&](const char* what) {
    CTX_LOCK(ctx);
    snprintf(ctx->err, sizeof(ctx->err), "same-message batch: %s", what);
    return -2;
  };
  if (const char* what = check_same_message(in, set_verdicts)) return bad(what);
  // the call as n one-set batchable requests over table indices, the job's root per set
  std::vector<uint32_t> off(n + 1);
  for (uint32_t i = 0; i <= n; ++i) off[i] = i;
  std::vector<uint8_t> batchable(n, 1), msgs(32ull * n);
  for (uint32_t j = 0; j < J; ++j)
    for (uint32_t i = in->job_set_offsets[j]; i < in->job_set_offsets[j + 1]; ++i)
      memcpy(&msgs[32ull * i], in->messages + 32ull * j, 32);
  SameMsgPlan sm;
  plan_same_message(in, sm);
  for (uint32_t r : sm.plan.nonbatch_reqs) batchable[r] = 0;
  bls_batch all;
  memset(&all, 0, sizeof(all));
  all.n_sets = n;
  all.n_reqs = n;
  all.req_set_offsets = off.data();
  all.req_batchable = batchable.data();
  all.set_pk_offsets = off.data();
  all.pk_indices = in->pk_indices;
  all.messages = msgs.data();
  all.signatures = in->signatures;
  all.seed = in->seed;
  PassArgs a{set_verdicts, stats};
  a.sm = &sm;
  return verify_impl(ctx, &all, a);
}

int bls_gpu_verify_deposits(bls_gpu_ctx* ctx, const bls_deposit_batch* in, int32_t* verdicts, bls_stats* stats) {
  if (!ctx || !in) return -2;
  const uint32_t n = in->n;
  if (n == 0) return 0;  // (nothing written, stats neither)
  if (stats) memset(stats, 0, sizeof(*stats));
  if (const char* what = check_deposits(in, verdicts)) {
    CTX_LOCK(ctx);
    snprintf(ctx->err, sizeof(ctx->err), "deposit batch: %s", what);
    return -2;
  }
  // the call as n one-set batchable requests (bls/plan.hpp plan_deposits); the front kernel
  // makes each one's key and signing root from the deposit's fields (PassArgs::dep), the
  // table is not consulted
  DepositPlan dp;
  bls_batch all;
  plan_deposits(in, dp, all);
  PassArgs a{verdicts, stats};
  a.dep = in;
  return verify_impl(ctx, &all, a);
}

int bls_gpu_partial(bls_gpu_ctx* ctx, const bls_batch* in, uint32_t set_index_base, uint8_t* out576,
                    int32_t* status, uint32_t* err_info, bls_stats* stats) {
  if (!in || !out576 || !status) return -2;
  if (in->seed == nullptr) {
    snprintf(ctx->err, sizeof(ctx->err), "bls_gpu_partial needs the call's shared seed");
    return -2;
  }
  static_assert(sizeof(Fp12) == 576, "Fp12 wire size");
  if (in->n_sets == 0 || in->n_reqs == 0) {
    snprintf(ctx->err, sizeof(ctx->err), "bls_gpu_partial: empty shard");
    return -2;
  }
  memset(out576, 0, 576);
  if (err_info) err_info[0] = 3, err_info[1] = 0;
  PassArgs a{nullptr, stats, set_index_base};
  a.partial_out = out576, a.partial_status = status, a.partial_err = err_info;
  return verify_impl(ctx, in, a);
}

int bls_gpu_final_check(bls_gpu_ctx* ctx, const uint8_t* partials, uint32_t n, int32_t* verdict) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  if (!partials || !verdict || n == 0) return -2;
  const uint32_t lvl1 = (n + FPROD_FAN - 1) / FPROD_FAN;
  Fp12 *in = nullptr, *t[2] = {nullptr, nullptr};
  int32_t* dv = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { c.buf(in, n).buf(t[0], lvl1).buf(t[1], lvl1).buf(dv, 1); })) return -1;
  HIPC(ctx, hipMemcpyAsync(in, partials, 576ull * n, hipMemcpyHostToDevice, run.s));
  if (fprod_tree(ctx, in, n, t, dv, nullptr, run.s)) return -1;
  HIPC(ctx, hipMemcpyAsync(verdict, dv, sizeof(int32_t), hipMemcpyDeviceToHost, run.s));
  return run.finish();
}

int bls_gpu_aggregate_pubkeys(bls_gpu_ctx* ctx, const uint32_t* set_pk_offsets, const uint32_t* pk_indices,
                              uint32_t n_sets, uint8_t* out96, int32_t* codes) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  if (n_sets == 0) return 0;
  uint32_t n_idx = set_pk_offsets[n_sets];
  std::vector<uint32_t> agg_list;
  for (uint32_t i = 0; i < n_sets; ++i)
    if (set_pk_offsets[i + 1] - set_pk_offsets[i] >= BLS_AGG_WAVE_MIN) agg_list.push_back(i);
  return aggregate_sets(
      ctx, n_sets, out96, codes,
      [&](Carver& c, PipeBufs& b) {
        c.buf(b.set_pk_off, n_sets + 1).buf(b.pk_idx, n_idx).buf(b.agg_sets, agg_list.size());
      },
      [&](PipeBufs& b, hipStream_t s) -> int {
        HIPC(ctx, hipMemcpyAsync((void*)b.set_pk_off, set_pk_offsets, sizeof(uint32_t) * (n_sets + 1),
                                 hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpyAsync((void*)b.pk_idx, pk_indices, sizeof(uint32_t) * n_idx, hipMemcpyHostToDevice, s));
        b.n_agg = (uint32_t)agg_list.size();
        b.agg_min = agg_list.empty() ? 0u : BLS_AGG_WAVE_MIN;
        if (!agg_list.empty()) {
          HIPC(ctx, hipMemcpyAsync((void*)b.agg_sets, agg_list.data(), sizeof(uint32_t) * agg_list.size(),
                                   hipMemcpyHostToDevice, s));
          HIPC(ctx, launch_k_pk_agg(b, s));  // the big aggregates first; k_aggregate serializes every set
        }
        return 0;
      });
}

int bls_gpu_aggregate_committee_bits(bls_gpu_ctx* ctx, const bls_committee_sets* cs, uint32_t n_sets, uint8_t* out96,
                                     int32_t* codes) {
  if (!ctx) return -2;
  CTX_LOCK(ctx);
  if (const int rc = committee_check_sets(cs, n_sets, nullptr, ctx->err, sizeof(ctx->err))) return rc;
  if (n_sets && !out96) return -2;
  for (uint32_t i = 0; i < n_sets; ++i)
    if (cs->set_committee[i] == BLS_SET_NO_COMMITTEE) {
      snprintf(ctx->err, sizeof(ctx->err), "committee sets: set %u names no committee", i);
      return -2;
    }
  HIPC(ctx, hipSetDevice(ctx->device));
  if (n_sets == 0) return 0;
  const uint32_t n_bytes = cs->set_bits_off[n_sets];
  std::vector<uint32_t> all(n_sets);
  for (uint32_t i = 0; i < n_sets; ++i) all[i] = i;
  return aggregate_sets(
      ctx, n_sets, out96, codes,
      [&](Carver& c, PipeBufs& b) {
        c.buf(b.set_committee, n_sets).buf(b.set_bits_off, n_sets + 1).buf(b.bits, n_bytes).buf(b.bits_sets, n_sets);
      },
      [&](PipeBufs& b, hipStream_t s) -> int {
        b.n_bits = n_sets;
        b.cm_groups = ctx->cm_dev;
        HIPC(ctx, hipMemcpyAsync((void*)b.set_committee, cs->set_committee, sizeof(uint32_t) * n_sets,
                                 hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpyAsync((void*)b.set_bits_off, cs->set_bits_off, sizeof(uint32_t) * (n_sets + 1),
                                 hipMemcpyHostToDevice, s));
        if (n_bytes) HIPC(ctx, hipMemcpyAsync((void*)b.bits, cs->bits, n_bytes, hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpyAsync((void*)b.bits_sets, all.data(), sizeof(uint32_t) * n_sets, hipMemcpyHostToDevice, s));
        HIPC(ctx, launch_k_pk_bits(b, s));
        return 0;
      });
}

int bls_gpu_aggregate_spans(bls_gpu_ctx* ctx, const bls_span_sets* ss, uint32_t n_sets, uint8_t* out96,
                            int32_t* codes) {
  if (!ctx) return -2;
  CTX_LOCK(ctx);
  if (const int rc = span_check_sets(ss, n_sets, false, nullptr, ctx->err, sizeof(ctx->err))) return rc;
  if (n_sets && !out96) {
    snprintf(ctx->err, sizeof(ctx->err), "span sets: out96 missing");
    return -2;
  }
  HIPC(ctx, hipSetDevice(ctx->device));
  if (n_sets == 0) return 0;
  const uint32_t n_refs = ss->set_span_off[n_sets], n_bytes = ss->set_bits_off[n_sets];
  std::vector<uint32_t> all(n_sets);
  for (uint32_t i = 0; i < n_sets; ++i) all[i] = i;
  return aggregate_sets(
      ctx, n_sets, out96, codes,
      [&](Carver& c, PipeBufs& b) {
        c.buf(b.set_span_off, n_sets + 1).buf(b.span_refs, n_refs).buf(b.set_bits_off, n_sets + 1);
        c.buf(b.bits, n_bytes).buf(b.span_sets, n_sets);
      },
      [&](PipeBufs& b, hipStream_t s) -> int {
        b.n_span = n_sets;
        b.cm_groups = ctx->cm_dev;
        HIPC(ctx, hipMemcpyAsync((void*)b.set_span_off, ss->set_span_off, sizeof(uint32_t) * (n_sets + 1),
                                 hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpyAsync((void*)b.span_refs, ss->span_refs, sizeof(uint32_t) * n_refs, hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpyAsync((void*)b.set_bits_off, ss->set_bits_off, sizeof(uint32_t) * (n_sets + 1),
                                 hipMemcpyHostToDevice, s));
        if (n_bytes) HIPC(ctx, hipMemcpyAsync((void*)b.bits, ss->bits, n_bytes, hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpyAsync((void*)b.span_sets, all.data(), sizeof(uint32_t) * n_sets, hipMemcpyHostToDevice, s));
        HIPC(ctx, launch_k_pk_span(b, s));
        return 0;
      });
}

static int run_simple(bls_gpu_ctx* ctx, uint32_t n, size_t in_a, const void* a, size_t in_b, const void* bsrc,
                      size_t out_per, void* out, int which) {
  HIPC(ctx, hipSetDevice(ctx->device));
  if (n == 0) return 0;
  uint8_t *d_a = nullptr, *d_b = nullptr, *d_o = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { c.buf(d_a, in_a * n).buf(d_b, in_b * n).buf(d_o, out_per * n); })) return -1;
  const hipStream_t s = run.s;
  HIPC(ctx, hipMemcpyAsync(d_a, a, in_a * n, hipMemcpyHostToDevice, s));
  if (in_b) HIPC(ctx, hipMemcpyAsync(d_b, bsrc, in_b * n, hipMemcpyHostToDevice, s));
  switch (which) {
    case 0: HIPC(ctx, launch_k_hash_to_g2(d_a, n, d_o, s)); break;
    case 1: HIPC(ctx, launch_k_sk_to_pk(d_a, n, d_o, s)); break;
    default: HIPC(ctx, launch_k_sign(d_a, d_b, n, d_o, s)); break;
  }
  HIPC(ctx, hipMemcpyAsync(out, d_o, out_per * n, hipMemcpyDeviceToHost, s));
  return run.finish();
}

int bls_gpu_aggregate_signatures(bls_gpu_ctx* ctx, const uint8_t* sigs96, const uint32_t* list_offsets,
                                 uint32_t n_lists, uint8_t* out96, int32_t* codes) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  if (n_lists == 0) return 0;
  if (!list_offsets || !out96 || !codes) return -2;
  const uint32_t n = list_offsets[n_lists];
  if (list_offsets[0] != 0) return -2;
  for (uint32_t l = 0; l < n_lists; ++l)
    if (list_offsets[l] > list_offsets[l + 1]) {
      snprintf(ctx->err, sizeof(ctx->err), "list_offsets not monotone at %u", l);
      return -2;
    }
  if (n > 0 && !sigs96) return -2;
  uint8_t *d_in = nullptr, *d_out = nullptr;
  uint32_t* d_off = nullptr;
  G2A* d_pts = nullptr;
  int32_t *d_sc = nullptr, *d_codes = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) {
        c.buf(d_in, 96ull * n).buf(d_off, n_lists + 1).buf(d_pts, n).buf(d_sc, n);
        c.buf(d_out, 96ull * n_lists).buf(d_codes, n_lists);
      }))
    return -1;
  const hipStream_t s = run.s;
  if (n) HIPC(ctx, hipMemcpyAsync(d_in, sigs96, 96ull * n, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemcpyAsync(d_off, list_offsets, sizeof(uint32_t) * (n_lists + 1), hipMemcpyHostToDevice, s));
  HIPC(ctx, launch_k_sig_aggregate(d_in, n, d_off, n_lists, d_pts, d_sc, d_out, d_codes, s));
  HIPC(ctx, hipMemcpyAsync(out96, d_out, 96ull * n_lists, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(codes, d_codes, sizeof(int32_t) * n_lists, hipMemcpyDeviceToHost, s));
  return run.finish();
}

int bls_gpu_g2_decompress(bls_gpu_ctx* ctx, const uint8_t* in96, uint32_t n, int validate, uint8_t* out192,
                          int32_t* codes) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  if (n == 0) return 0;
  if (!in96 || !out192 || !codes) return -2;
  uint8_t *d_in = nullptr, *d_out = nullptr;
  int32_t* d_codes = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { c.buf(d_in, 96ull * n).buf(d_out, 192ull * n).buf(d_codes, n); })) return -1;
  const hipStream_t s = run.s;
  HIPC(ctx, hipMemcpyAsync(d_in, in96, 96ull * n, hipMemcpyHostToDevice, s));
  HIPC(ctx, launch_k_g2_decompress(d_in, n, validate, d_out, d_codes, s));
  HIPC(ctx, hipMemcpyAsync(out192, d_out, 192ull * n, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(codes, d_codes, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  return run.finish();
}

int bls_gpu_ssz_roots(bls_gpu_ctx* ctx, uint32_t kind, const uint8_t* objs, uint32_t n, const uint8_t* domains,
                      uint32_t domain_stride, uint8_t* out32) {
  CTX_LOCK(ctx);
  if (!ssz_kind_known(kind) || (domains && domain_stride != 0 && domain_stride != 32)) {
    snprintf(ctx->err, sizeof(ctx->err), "bls_gpu_ssz_roots: unknown kind 0x%x or domain stride %u", kind,
             domain_stride);
    return -2;
  }
  HIPC(ctx, hipSetDevice(ctx->device));
  if (n == 0) return 0;
  if (!objs || !out32) return -2;
  const size_t obj_bytes = (size_t)BLS_SSZ_SIZE(kind) * n, dom_bytes = domains ? (domain_stride ? 32ull * n : 32) : 0;
  uint8_t *d_obj = nullptr, *d_dom = nullptr, *d_out = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { c.buf(d_obj, obj_bytes).buf(d_dom, dom_bytes).buf(d_out, 32ull * n); })) return -1;
  const hipStream_t s = run.s;
  HIPC(ctx, hipMemcpyAsync(d_obj, objs, obj_bytes, hipMemcpyHostToDevice, s));
  if (domains) HIPC(ctx, hipMemcpyAsync(d_dom, domains, dom_bytes, hipMemcpyHostToDevice, s));
  HIPC(ctx, launch_k_ssz_roots(kind, d_obj, n, domains ? d_dom : nullptr, domain_stride, d_out, s));
  HIPC(ctx, hipMemcpyAsync(out32, d_out, 32ull * n, hipMemcpyDeviceToHost, s));
  return run.finish();
}

int bls_gpu_hash_to_g2(bls_gpu_ctx* ctx, const uint8_t* msgs, uint32_t n, uint8_t* out192) {
  CTX_LOCK(ctx);
  return run_simple(ctx, n, 32, msgs, 0, nullptr, 192, out192, 0);
}

int bls_gpu_sk_to_pk(bls_gpu_ctx* ctx, const uint8_t* sks, uint32_t n, uint8_t* out48) {
  CTX_LOCK(ctx);
  return run_simple(ctx, n, 32, sks, 0, nullptr, 48, out48, 1);
}

int bls_gpu_sign(bls_gpu_ctx* ctx, const uint8_t* sks, const uint8_t* msgs, uint32_t n, uint8_t* out96) {
  CTX_LOCK(ctx);
  return run_simple(ctx, n, 32, sks, 32, msgs, 96, out96, 2);
}

}  // extern "C"

extern "C" int bls_gpu_set_debug_flags(bls_gpu_ctx* ctx, uint32_t flags) {
  if (!ctx) return -1;
  ctx->debug_flags = flags;
  return 0;
}

extern "C" int bls_gpu_group_test_counts(bls_gpu_ctx* ctx, uint32_t out[8]) {
  if (!ctx || !out) return -2;
  CTX_LOCK(ctx);
  memcpy(out, ctx->gt_counts, sizeof(ctx->gt_counts));
  return 0;
}

extern "C" int bls_gpu_mad_peak(bls_gpu_ctx* ctx, double* mads_per_s, double* ms_out) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  int cus = 0;
  HIPC(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const uint32_t blocks = (uint32_t)cus * 8, iters = 1024;
  uint64_t* d = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { d = c.take<uint64_t>(blocks); })) return -1;
  const hipStream_t s = run.s;
  HIPC(ctx, launch_k_mad_peak(d, blocks, iters, s));  // warm-up (clocks, code load)
  HIPC(ctx, hipEventRecord(ctx->ev0, s));
  HIPC(ctx, launch_k_mad_peak(d, blocks, iters, s));
  HIPC(ctx, hipEventRecord(ctx->ev1, s));
  if (run.finish()) return -1;
  float ms = 0.f;
  HIPC(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  double mads = (double)blocks * 256.0 * iters * 16.0 * 8.0;
  *mads_per_s = mads / (ms * 1e-3);
  if (ms_out) *ms_out = ms;
  return 0;
}

extern "C" int bls_gpu_fp_mul_test(bls_gpu_ctx* ctx, const uint8_t* a48, const uint8_t* b48, uint32_t n,
                                   uint8_t* out48) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  if (n == 0) return 0;
  const size_t sz = 48ull * n;
  uint8_t *da = nullptr, *db = nullptr, *dout = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { c.buf(da, sz).buf(db, sz).buf(dout, sz); })) return -1;
  const hipStream_t s = run.s;
  HIPC(ctx, hipMemcpyAsync(da, a48, sz, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemcpyAsync(db, b48, sz, hipMemcpyHostToDevice, s));
  HIPC(ctx, launch_k_fp_mul_test(da, db, n, dout, s));
  HIPC(ctx, hipMemcpyAsync(out48, dout, sz, hipMemcpyDeviceToHost, s));
  return run.finish();
}

// The body of the field, curve and tower op self-tests: n records of iw words in, n of ow
// words out (zeroed before the launch), and behind them ws_bytes of zeroed workspace (curve
// ops; none: `launch` gets nullptr).  `launch` names the op's kernel launcher.
template <class Launch>
static int op_test(bls_gpu_ctx* ctx, uint32_t iw, uint32_t ow, size_t ws_bytes, const uint32_t* in, uint32_t n,
                   uint32_t* out, Launch&& launch) {
  const size_t in_sz = 4ull * iw * n, out_sz = 4ull * ow * n;
  uint32_t *din = nullptr, *dout = nullptr;
  uint8_t* dws = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { c.buf(din, (size_t)iw * n).buf(dout, (size_t)ow * n).buf(dws, ws_bytes); })) return -1;
  HIPC(ctx, hipMemcpyAsync(din, in, in_sz, hipMemcpyHostToDevice, run.s));
  HIPC(ctx, hipMemsetAsync(dout, 0, out_sz, run.s));
  if (ws_bytes) HIPC(ctx, hipMemsetAsync(dws, 0, ws_bytes, run.s));
  if (const int rc = launch(din, dout, ws_bytes ? dws : nullptr, run.s)) return rc;
  HIPC(ctx, hipMemcpyAsync(out, dout, out_sz, hipMemcpyDeviceToHost, run.s));
  return run.finish();
}

// The chain rows (PipeBufs::chain) of n records of iw words that begin with RP (x, y, z) and
// HQ (x.c0, x.c1, y.c0, y.c1): the two at their CH_RP and CH_HQ slots, every other slot zero.
static std::vector<uint32_t> chain_rows(const uint32_t* in, uint32_t iw, uint32_t n) {
  std::vector<uint32_t> chain((size_t)CHAIN_WORDS * 12 * n, 0u);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* r = in + (size_t)iw * i;
    uint32_t* row = chain.data() + (size_t)CHAIN_WORDS * 12 * i;
    memcpy(row + 12 * CH_RP, r, 4 * 36);
    memcpy(row + 12 * CH_HQ, r + 36, 4 * 48);
  }
  return chain;
}

extern "C" int bls_gpu_field_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words) {
  return field_op_shape(op, in_words, out_words);
}

// One field primitive per lane on raw words (kernels/field_ops.hpp): n records of the
// op's in_words in, n of its out_words out.
extern "C" int bls_gpu_field_op_test(bls_gpu_ctx* ctx, uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  uint32_t iw = 0, ow = 0;
  if (field_op_shape(op, &iw, &ow) != 0) {
    snprintf(ctx->err, sizeof(ctx->err), "unknown field op 0x%x", op);
    return -2;
  }
  if (n == 0) return 0;
  return op_test(ctx, iw, ow, 0, in, n, out, [&](const uint32_t* din, uint32_t* dout, void*, hipStream_t s) -> int {
    HIPC(ctx, launch_k_field_op(op, din, n, dout, s));
    return 0;
  });
}

extern "C" int bls_gpu_curve_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words) {
  return curve_op_shape(op, in_words, out_words);
}

// COP_MILLER: the split SIMT Miller loops through launch_k_mlqf on a zero-initialised
// PipeBufs that holds only what the launched kernels read.  Record: RP (x, y, z: Jacobian
// G1, any z), HQ (x.c0, x.c1, y.c0, y.c1), the item's product domain, per_lane (record 0's
// counts: 1, 2, 4 or MLF_PAIR); out: f[i].  PipeBufs fields dereferenced (kernels/k_mlq.hip):
//   ml_live    chain_live[i]; set_unit only when non-null (left null); n_sets by value
//   mlq_lane   chain (CH_RP, CH_HQ), the line buffer
//   mlf_lane   ml_dom[i] (when non-null), indiv_vbase by value, f[i], the line buffer
//   k_mlf2     f[i], the line buffer
// and launch_k_mlqf reads mlf_pl on the host.  msg_rep, set_unit and everything else stay null.
static int curve_miller_test(bls_gpu_ctx* ctx, const uint32_t* in, uint32_t n, uint32_t* out) {
  const uint32_t iw = (uint32_t)curve_op_in_words(COP_MILLER), per_lane = in[iw - 1];
  if (n > COP_MILLER_MAX || !(per_lane == 1 || per_lane == 2 || per_lane == 4 || per_lane == MLF_PAIR)) {
    snprintf(ctx->err, sizeof(ctx->err), "curve op MILLER: %u items, per_lane %u", n, per_lane);
    return -2;
  }
  const std::vector<uint32_t> chain = chain_rows(in, iw, n), live(n, 1u);
  std::vector<uint32_t> dom(n);
  for (uint32_t i = 0; i < n; ++i) dom[i] = in[(size_t)iw * i + 84];
  PipeBufs b;
  memset(&b, 0, sizeof(b));
  b.n_sets = n;
  b.indiv_vbase = n;
  b.mlf_pl = per_lane;
  uint32_t* lines = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) {
        c.buf(b.chain, (size_t)CHAIN_WORDS * n).buf(b.chain_live, n).buf(b.ml_dom, n).buf(b.f, n);
        c.buf(lines, mlq_line_words(n));
      }))
    return -1;
  const hipStream_t s = run.s;
  HIPC(ctx, hipMemcpyAsync(b.chain, chain.data(), 4 * chain.size(), hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemcpyAsync(b.chain_live, live.data(), 4ull * n, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemcpyAsync((void*)b.ml_dom, dom.data(), 4ull * n, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemsetAsync(b.f, 0, sizeof(Fp12) * (size_t)n, s));
  HIPC(ctx, launch_k_mlqf(b, 0, n, false, lines, s));
  HIPC(ctx, hipMemcpyAsync(out, b.f, sizeof(Fp12) * (size_t)n, hipMemcpyDeviceToHost, s));
  return run.finish();
}

// COP_FE: FE(F) == 1 for n Fp12 values, each its own one-request, one-set chunk, through the
// SIMT chunk kernel and through the cooperative one over the same buffers; out: chunk_ok of
// each form.  PipeBufs fields dereferenced (k_chunk_simt, k_chunk_coop):
//   n_chunks by value; chunk_off[c], chunk_off[c + 1]; chunk_reqs[k]; req_status[r];
//   req_off[r], req_off[r + 1]; f[i]; chunk_ok[c]; set_unit, unit_off, chunk_fe only when
//   non-null (left null); sigagg = 0, so n_sets and unit_base are not used
// plus the SIMT form's four Fp12 of save per task and the context's program table.
static int curve_fe_test(bls_gpu_ctx* ctx, const uint32_t* in, uint32_t n, uint32_t* out) {
  std::vector<uint32_t> idx(n + 1);
  for (uint32_t i = 0; i <= n; ++i) idx[i] = i;
  std::vector<int32_t> ok(2 * (size_t)n);
  PipeBufs b;
  memset(&b, 0, sizeof(b));
  b.n_chunks = n;
  b.n_reqs = n;
  b.n_sets = n;
  Fp12* save = nullptr;
  uint32_t* d_idx = nullptr;
  int32_t *ok_simt = nullptr, *ok_coop = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) {
        c.buf(b.f, n).buf(save, 4ull * n).buf(d_idx, n + 1).buf(b.req_status, n).buf(ok_simt, n).buf(ok_coop, n);
      }))
    return -1;
  b.chunk_off = b.chunk_reqs = b.req_off = d_idx;  // chunk c = request c = set c
  const hipStream_t s = run.s;
  HIPC(ctx, hipMemcpyAsync(b.f, in, sizeof(Fp12) * (size_t)n, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemcpyAsync(d_idx, idx.data(), 4ull * (n + 1), hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemsetAsync(b.req_status, 0, 4ull * n, s));
  HIPC(ctx, hipMemsetAsync(ok_simt, 0xFF, 4ull * n, s));  // -1: a kernel that writes nothing shows
  HIPC(ctx, hipMemsetAsync(ok_coop, 0xFF, 4ull * n, s));
  b.chunk_ok = ok_simt;
  HIPC(ctx, launch_k_chunk_simt(b, save, s));
  b.chunk_ok = ok_coop;
  HIPC(ctx, launch_k_chunk_coop(b, ctx->coop, s));
  HIPC(ctx, hipMemcpyAsync(ok.data(), ok_simt, 4ull * n, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(ok.data() + n, ok_coop, 4ull * n, hipMemcpyDeviceToHost, s));
  if (run.finish()) return -1;
  for (uint32_t i = 0; i < n; ++i) {
    out[2 * i] = (uint32_t)ok[i];
    out[2 * i + 1] = (uint32_t)ok[n + i];
  }
  return 0;
}

// One curve-level function per lane on Montgomery-form words (kernels/curve_ops.hpp): n
// records of the op's in_words in, n of its out_words out; chain_role_h's rows and bytes
// live in zeroed workspace behind them.
extern "C" int bls_gpu_curve_op_test(bls_gpu_ctx* ctx, uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  uint32_t iw = 0, ow = 0;
  if (curve_op_shape(op, &iw, &ow) != 0) {
    snprintf(ctx->err, sizeof(ctx->err), "unknown curve op 0x%x", op);
    return -2;
  }
  if (n == 0) return 0;
  if ((op & ~COP_D28_FLAG) == COP_MILLER) return curve_miller_test(ctx, in, n, out);
  if ((op & ~COP_D28_FLAG) == COP_FE) return curve_fe_test(ctx, in, n, out);
  return op_test(ctx, iw, ow, curve_op_ws_bytes(op, n), in, n, out,
                 [&](const uint32_t* din, uint32_t* dout, void* dws, hipStream_t s) -> int {
                   HIPC(ctx, launch_k_curve_op(op, din, n, dout, dws, s));
                   return 0;
                 });
}

extern "C" int bls_gpu_tower_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words) {
  return tower_op_shape(op, in_words, out_words);
}

// TOP_MLQ_LINES: k_mlq<1> alone (launch_k_mlq_lines) on a zero-initialised PipeBufs that
// holds only what mlq_lane reads -- chain (CH_RP, CH_HQ) and chain_live[i]; units_paired = 0,
// so set_unit stays null -- and a zeroed line buffer.  Record: RP (x, y, z: Jacobian G1, any
// z != 0), HQ (x.c0, x.c1, y.c0, y.c1); out: item k's 68 lines, event-major, each l0, l2, l3
// as store_line wrote them (the buffer itself is line-major and lane-minor).
static int tower_lines_test(bls_gpu_ctx* ctx, const uint32_t* in, uint32_t n, uint32_t* out) {
  if (n > TOP_LINES_MAX) {
    snprintf(ctx->err, sizeof(ctx->err), "tower op MLQ_LINES: %u items (at most %u)", n, TOP_LINES_MAX);
    return -2;
  }
  const uint32_t iw = 12u * (uint32_t)tower_op_in_fps(TOP_MLQ_LINES), ow = 12u * (uint32_t)tower_op_out_fps(TOP_MLQ_LINES);
  const std::vector<uint32_t> chain = chain_rows(in, iw, n), live(n, 1u);
  const size_t words = mlq_line_words(n), stride = words / ow;
  std::vector<uint32_t> buf(words);
  PipeBufs b;
  memset(&b, 0, sizeof(b));
  b.n_sets = n;
  uint32_t* lines = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { c.buf(b.chain, (size_t)CHAIN_WORDS * n).buf(b.chain_live, n).buf(lines, words); }))
    return -1;
  const hipStream_t s = run.s;
  HIPC(ctx, hipMemcpyAsync(b.chain, chain.data(), 4 * chain.size(), hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemcpyAsync(b.chain_live, live.data(), 4ull * n, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemsetAsync(lines, 0, 4 * words, s));
  HIPC(ctx, launch_k_mlq_lines(b, n, lines, s));
  HIPC(ctx, hipMemcpyAsync(buf.data(), lines, 4 * words, hipMemcpyDeviceToHost, s));
  if (run.finish()) return -1;
  for (uint32_t k = 0; k < n; ++k)
    for (uint32_t ew = 0; ew < ow; ++ew) out[(size_t)ow * k + ew] = buf[(size_t)ew * stride + k];
  return 0;
}

// One tower function per lane on Montgomery-form words (kernels/tower_ops.hpp): n records of
// the op's in_words in, n of its out_words out.  An op in a flavour it does not exist in
// returns -2 before anything is launched or written.
extern "C" int bls_gpu_tower_op_test(bls_gpu_ctx* ctx, uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  uint32_t iw = 0, ow = 0;
  if (tower_op_shape(op, &iw, &ow) != 0) {
    snprintf(ctx->err, sizeof(ctx->err), "unknown tower op 0x%x", op);
    return -2;
  }
  if (n == 0) return 0;
  if ((op & ~TOP_D28_FLAG) == TOP_MLQ_LINES) return tower_lines_test(ctx, in, n, out);
  return op_test(ctx, iw, ow, 0, in, n, out, [&](const uint32_t* din, uint32_t* dout, void*, hipStream_t s) -> int {
    HIPC(ctx, launch_k_tower_op(op, din, n, dout, s));
    return 0;
  });
}

// Dependent Montgomery-product chain: `lanes` lanes (multiple of 64) x `iters` products.
// ns_per_fpm = wall time / iters (per-lane latency); fpm_per_s = lanes * iters / time.
extern "C" int bls_gpu_fpm_bench(bls_gpu_ctx* ctx, uint32_t lanes, uint32_t iters, double* ns_per_fpm,
                                 double* fpm_per_s) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  lanes = (lanes + 63) / 64 * 64;
  Fp* io = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { io = c.take<Fp>(2ull * lanes); })) return -1;
  const hipStream_t s = run.s;
  HIPC(ctx, hipMemsetAsync(io, 0x11, sizeof(Fp) * 2 * lanes, s));
  HIPC(ctx, launch_k_fpm_chain(io, lanes, 8, s));
  HIPC(ctx, hipEventRecord(ctx->ev0, s));
  HIPC(ctx, launch_k_fpm_chain(io, lanes, iters, s));
  HIPC(ctx, hipEventRecord(ctx->ev1, s));
  if (run.finish()) return -1;
  float ms = 0.f;
  HIPC(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *ns_per_fpm = ms * 1e6 / iters;
  *fpm_per_s = (double)lanes * iters / (ms * 1e-3);
  return 0;
}

extern "C" int bls_gpu_kernel_probe(bls_gpu_ctx* ctx, const char* name, uint32_t lanes, uint32_t reps, double* ms) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  const size_t per = name ? kernel_probe_out_bytes(name) : 0;
  if (!per || !ms || lanes == 0) {
    snprintf(ctx->err, sizeof(ctx->err), "unknown probe %s", name ? name : "(null)");
    return -2;
  }
  uint8_t* d = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { d = c.take<uint8_t>(per * lanes); })) return -1;
  const hipStream_t s = run.s;
  HIPC(ctx, launch_kernel_probe(name, d, lanes, s));  // warm-up
  HIPC(ctx, hipEventRecord(ctx->ev0, s));
  for (uint32_t r = 0; r < reps; ++r) HIPC(ctx, launch_kernel_probe(name, d, lanes, s));
  HIPC(ctx, hipEventRecord(ctx->ev1, s));
  if (run.finish()) return -1;
  float t = 0.f;
  HIPC(ctx, hipEventElapsedTime(&t, ctx->ev0, ctx->ev1));
  *ms = t;
  return 0;
}

// The cooperative program `name` of the loaded table and, with `frame`, its frame size in
// slots; a null or unknown name: -1 and "no program ...".
static int coop_lookup(bls_gpu_ctx* ctx, const char* name, CoopProg* pg, uint32_t* frame) {
  bool found = false;
  for (size_t k = 0; name && k < ctx->coop_progs->size(); ++k)
    if ((*ctx->coop_progs)[k].first == name) {
      *pg = (*ctx->coop_progs)[k].second;
      if (frame) *frame = (*ctx->coop_frames)[k];
      found = true;
    }
  if (found) return 0;
  snprintf(ctx->err, sizeof(ctx->err), "no program %s", name ? name : "(null)");
  return -1;
}

// Probe: time the cooperative program `name` (blocks x reps runs); us_per_step is the
// wall time of one run divided by its step count.
extern "C" int bls_gpu_coop_probe(bls_gpu_ctx* ctx, const char* name, uint32_t blocks, uint32_t reps,
                                  double* us_per_step, double* ms_total, uint64_t* step_stamps) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  CoopProg pg{0, 0};
  if (const int rc = coop_lookup(ctx, name, &pg, nullptr)) return rc;
  uint32_t* sink = nullptr;
  uint64_t* d_stamps = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) { c.buf(sink, blocks).buf(d_stamps, 2ull * pg.n + 1); })) return -1;
  hipStream_t s = run.s;
  HIPC(ctx, launch_k_coop_probe(ctx->coop, pg, blocks, 1, sink, nullptr, s));
  HIPC(ctx, hipEventRecord(ctx->ev0, s));
  HIPC(ctx, launch_k_coop_probe(ctx->coop, pg, blocks, reps, sink, nullptr, s));
  HIPC(ctx, hipEventRecord(ctx->ev1, s));
  if (run.finish()) return -1;
  float ms = 0.f;
  HIPC(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *us_per_step = ms * 1e3 / ((double)reps * pg.n);
  if (ms_total) *ms_total = ms;
  if (step_stamps) {  // one more run of block 0 with s_memtime stamps: step start, compute done
    // (or the point $BLS_COOP_PROBE_MARK names, coop.hpp coop_step; steps that do not
    // reach it keep 0)
    const char* me = getenv("BLS_COOP_PROBE_MARK");
    const uint64_t mark = me ? strtoull(me, nullptr, 10) : 0ull;
    OneShot stamps(ctx);  // (the layout is the timed run's)
    HIPC(ctx, hipMemsetAsync(d_stamps, 0, 8ull * (2 * pg.n + 1), s));
    HIPC(ctx, hipMemcpyAsync(d_stamps, &mark, 8, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipStreamSynchronize(s));
    HIPC(ctx, launch_k_coop_probe(ctx->coop, pg, 1, 0, sink, d_stamps, s));
    HIPC(ctx, hipMemcpyAsync(step_stamps, d_stamps, 8ull * (2 * pg.n + 1), hipMemcpyDeviceToHost, s));
    return stamps.finish();
  }
  return 0;
}

// Test: program `name` of the loaded table run once on each of n_frames caller frames of
// n_slots raw Fp values (12 little-endian words each); frames_out gets the raw frames
// after the run, flags_out one zero-check flag word per frame.  n_slots must be the
// program's frame size in the table (-2 otherwise: the constant bank sits behind it).
extern "C" int bls_gpu_coop_run_test(bls_gpu_ctx* ctx, const char* name, const uint32_t* frames_in, uint32_t n_frames,
                                     uint32_t n_slots, uint32_t* frames_out, uint32_t* flags_out) {
  CTX_LOCK(ctx);
  HIPC(ctx, hipSetDevice(ctx->device));
  CoopProg pg{0, 0};
  uint32_t frame = 0;
  if (const int rc = coop_lookup(ctx, name, &pg, &frame)) return rc;
  if (n_slots != frame || (frame != COOP_FRAME && frame != COOP_FRAME2 && frame != COOP_FRAME3)) {
    snprintf(ctx->err, sizeof(ctx->err), "program %s has a frame of %u slots, not %u", name, frame, n_slots);
    return -2;
  }
  if (n_frames == 0) return 0;
  const std::string nm(name);
  const bool w2 = nm.size() > 3 && nm.compare(nm.size() - 3, 3, "_w2") == 0;  // two-wavefront programs
  const size_t fr_sz = sizeof(Fp) * (size_t)frame * n_frames;
  Fp *din = nullptr, *dout = nullptr;
  uint32_t* dflags = nullptr;
  OneShot run(ctx);
  if (run.carve([&](Carver& c) {
        c.buf(din, (size_t)frame * n_frames).buf(dout, (size_t)frame * n_frames).buf(dflags, n_frames);
      }))
    return -1;
  const hipStream_t s = run.s;
  HIPC(ctx, hipMemcpyAsync(din, frames_in, fr_sz, hipMemcpyHostToDevice, s));
  HIPC(ctx, launch_k_coop_run_test(ctx->coop, pg, frame, w2, din, n_frames, dout, dflags, s));
  HIPC(ctx, hipMemcpyAsync(frames_out, dout, fr_sz, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(flags_out, dflags, 4ull * n_frames, hipMemcpyDeviceToHost, s));
  return run.finish();
}
