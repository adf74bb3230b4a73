// The BLS_* environment knobs that choose a verify pass's shape: one table, parsed once
// into one struct, and the decisions taken from it.  Plain C++ (no HIP header, no
// context); the decisions are pure -- the process-wide count of sets in flight comes in
// as an argument -- so each is checked on the CPU (tests/native/plan_exports.hpp,
// tests/test_knobs_cpu.py, and under sanitizers tests/native/plan_host.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/lodestar_bls.h"
#include "plan_shape.hpp"

namespace bls {

// How a variable's text becomes its value (knob_value)
enum KnobKind {
  KNOB_FORCE,        // atoi; >= 0 forces (0 off, else on), negative = unset (-1)
  KNOB_U64,          // strtoull
  KNOB_U32,          // strtoul, kept as uint32_t
  KNOB_INT,          // atoi
  KNOB_SET,          // set at all (even empty) = 1
  KNOB_GT_MIN,       // atol; <= 0 -> 0xFFFFFFFF (off), 1 -> 2
  KNOB_ON_UNLESS_0,  // 0 iff set and atoi == 0
  KNOB_ON_UNLESS_1,  // 0 iff set and atoi == 1
  KNOB_DIGIT01,      // first char '0' / '1' forces; anything else = unset (-1)
  KNOB_SYNC,         // "spin" -> 1, "poll" -> 2, else 0
  KNOB_WAVES,        // 1 iff atoi == 1, else 2
  KNOB_PER_LANE,     // atoi in {1, 2, 4, MLF_PAIR}, else 0
  KNOB_PACK,         // atoi in 1 .. 3, else 0
};

// the per-set kernel packs 2 or 3 sets per wavefront from this many sets on (pack_for)
#define BLS_PACK_MIN_SETS 512u

// X(variable, field type, field, parse kind, value when unset, description): the one list
// of the knobs.  INTEGRATION.md's table carries every name (tests/test_knobs_cpu.py).
#define BLS_KNOB_TABLE(X)                                                                                              \
  X("BLS_SIGAGG", int, sigagg, KNOB_FORCE, -1, "0 / 1 forces the per-set / the aggregated-signature first pass")      \
  X("BLS_PERSET_MAX_INFLIGHT", uint64_t, perset_max_inflight, KNOB_U64, 20480,                                         \
    "sets in flight up to which calls of 512 .. 2,048 sets take the per-set path")                                     \
  X("BLS_DEBUG_SYNC", bool, debug_sync, KNOB_SET, 0,                                                                   \
    "set: synchronise after every kernel of a verify call and log its name and time")                                  \
  X("BLS_GROUP_TEST_MIN", uint32_t, group_test_min, KNOB_GT_MIN, 4,                                                    \
    "smallest failed chunk that is group-tested (0 = off)")                                                            \
  X("BLS_GROUP_SUMS", bool, group_sums, KNOB_ON_UNLESS_0, 1, "0: no group test pairs a signature sum of its own")      \
  X("BLS_GROUP_SUMS_MIN", uint64_t, group_sums_min, KNOB_U64, 512,                                                     \
    "group-tested requests in a pass from which the group tests take group sums")                                      \
  X("BLS_GROUP_EQ", int, group_eq, KNOB_INT, 1,                                                                        \
    "complement inference in the group tests: 0 two rounds without it, 2 always tests the whole chunk")                \
  X("BLS_MSM", int, msm, KNOB_DIGIT01, -1, "1 / 0 forces the Pippenger merged signature sum on / off")                 \
  X("BLS_MSM_MIN", uint64_t, msm_min, KNOB_U64, 60000, "sets in flight above which the Pippenger sum runs")            \
  X("BLS_MSM_OVERLAP", bool, msm_overlap, KNOB_ON_UNLESS_0, 1,                                                         \
    "0: the Pippenger sum as launches of its own in front of the Miller loops, not inside them")                       \
  X("BLS_ML_SHARED", bool, ml_shared, KNOB_ON_UNLESS_0, 1, "0: no shared Miller loops per product domain")             \
  X("BLS_SIG_TOTAL", bool, sig_total, KNOB_ON_UNLESS_0, 1,                                                             \
    "0: one signature sum per chunk under the merged check, not one per pass")                                         \
  X("BLS_MERGED_AFTER_FAIL", bool, merged_skip_after_fail, KNOB_ON_UNLESS_1, 1,                                        \
    "1: the merged check on every pass, also after one that failed it")                                                \
  X("BLS_SYNC", int, sync, KNOB_SYNC, 0, "spin / poll: how the host thread waits for a pass, whatever its size")       \
  X("BLS_MLF2_WAVES", uint32_t, mlf2_waves, KNOB_WAVES, 2, "wavefronts per SIMD of the two-lane f side (k_mlf2)")      \
  X("BLS_MLF_PER_LANE", uint32_t, mlf_per_lane, KNOB_PER_LANE, 0,                                                      \
    "1, 2, 4: items per k_mlf lane; 3: two lanes per item (k_mlf2)")                                                   \
  X("BLS_MLF_PAIR_MAX", uint64_t, mlf_pair_max, KNOB_U64, 16384,                                                       \
    "sets in flight (later loops: items) up to which the f side runs two lanes per item")                              \
  X("BLS_MLF_PL2_MIN", uint64_t, mlf_pl2_min, KNOB_U64, 98304, "sets in flight above which two items share a k_mlf lane") \
  X("BLS_MLF_PL4_MIN", uint64_t, mlf_pl4_min, KNOB_U64, 200000, "sets in flight above which four items share a k_mlf lane") \
  X("BLS_MLF_ALONE", bool, mlf_alone, KNOB_ON_UNLESS_0, 1,                                                             \
    "0: a failing pass's later Miller loops keep the first pass's items per lane")                                     \
  X("BLS_PACK", uint32_t, pack, KNOB_PACK, 0, "1, 2, 3: sets per wavefront of the per-set kernel")                     \
  X("BLS_PACK_MIN", uint32_t, pack_min, KNOB_U32, BLS_PACK_MIN_SETS,                                                   \
    "sets from which the per-set kernel packs 2 or 3 sets per wavefront")                                              \
  X("BLS_PACK3_INFLIGHT", uint64_t, pack3_inflight, KNOB_U64, 2048,                                                    \
    "sets in flight above which the per-set kernel packs 3 sets per wavefront, not 2")                                 \
  X("BLS_COOP_ML_MAX", uint32_t, coop_ml_max, KNOB_U32, 8192,                                                          \
    "items up to which a failing pass's later Miller loops run one wavefront per item (0 = never)")                    \
  X("BLS_INDIV2_MAX", uint32_t, indiv2_max, KNOB_U32, 64,                                                              \
    "requests verified alone up to which each takes two wavefronts (k_indiv_coop2)")                                   \
  X("BLS_FE_SIMT_MIN", uint32_t, fe_simt_min, KNOB_U32, 0,                                                             \
    "tasks from which a failing pass's final exponentiations run one lane per task (0 = never)")

struct Knobs {
#define X(name, type, field, kind, unset, doc) type field;
  BLS_KNOB_TABLE(X)
#undef X
};

struct KnobRow {
  const char *name, *doc;
};
inline const KnobRow* knob_rows(size_t* n) {
  static const KnobRow rows[] = {
#define X(name, type, field, kind, unset, doc) {name, doc},
      BLS_KNOB_TABLE(X)
#undef X
  };
  *n = sizeof(rows) / sizeof(rows[0]);
  return rows;
}

// the value of a variable whose text is e (nullptr: unset)
inline long long knob_value(KnobKind kind, const char* e, long long unset) {
  if (kind == KNOB_SET) return e != nullptr;
  if (kind == KNOB_ON_UNLESS_0) return !(e && atoi(e) == 0);
  if (kind == KNOB_ON_UNLESS_1) return !(e && atoi(e) == 1);
  if (kind == KNOB_DIGIT01) return e && (e[0] == '0' || e[0] == '1') ? e[0] - '0' : -1;
  if (kind == KNOB_SYNC) return e && !strcmp(e, "spin") ? 1 : e && !strcmp(e, "poll") ? 2 : 0;
  if (kind == KNOB_WAVES) return e && atoi(e) == 1 ? 1 : 2;
  if (kind == KNOB_GT_MIN) {
    const long x = e ? atol(e) : (long)unset;
    return x <= 0 ? 0xFFFFFFFFll : (uint32_t)(x < 2 ? 2 : x);
  }
  if (!e) return unset;
  if (kind == KNOB_U64) return (long long)strtoull(e, nullptr, 10);
  if (kind == KNOB_U32) return (uint32_t)strtoul(e, nullptr, 10);
  const int v = atoi(e);
  if (kind == KNOB_FORCE) return v >= 0 ? v : -1;
  if (kind == KNOB_PER_LANE) return (v == 1 || v == 2 || v == 4 || v == (int)MLF_PAIR) ? v : 0;
  if (kind == KNOB_PACK) return (v >= 1 && v <= 3) ? v : 0;
  return v;  // KNOB_INT
}

inline Knobs knobs_parse(const char* (*get)(const char*)) {
  Knobs k;
#define X(name, type, field, kind, unset, doc) k.field = (type)knob_value(kind, get(name), (long long)(unset));
  BLS_KNOB_TABLE(X)
#undef X
  return k;
}

// the process's knobs: the environment as it is at the first use
inline const Knobs& knobs() {
  static const Knobs k = knobs_parse([](const char* name) -> const char* { return getenv(name); });
  return k;
}

// Which first pass a call takes.  Aggregated-signature path (k_chain + k_gsum + k_vset + k_mln single-pair Miller
// loops, one signature Miller loop per chunk) from SIGAGG_MIN_SETS sets on, except for
// calls of at most PERSET_MAX_CALL sets while the process has at most
// $BLS_PERSET_MAX_INFLIGHT (20,480) sets in flight (this call's included): those run the
// all-cooperative k_pset / k_psetn (a set's chains spread over a wavefront instead of one
// lane: shorter calls while the device has room, fewer sets per second once it is full --
// per-set vs aggregated at 12 x 1024-set calls in flight 0.82M vs 0.56M sets/s, 16 x 1024
// 0.82M vs 0.72M, 24 x 1024 1.02M vs 1.03M, profiles/r04_ab_perset_crossover.json).  A call of more sets would fill
// every SIMD with its wavefronts (2 sets each, two per SIMD) and hold the main-thread
// lane's context behind it (test_napi.py: a 4096-set pool call finished first).
// BLS_DEBUG_SIGAGG_ON / _OFF or $BLS_SIGAGG (0 / 1) force a path.
#define SIGAGG_MIN_SETS 512u
#define PERSET_MAX_CALL 2048u
inline bool use_sigagg(const Knobs& k, uint32_t debug_flags, uint32_t n, uint64_t in_flight) {
  if (debug_flags & BLS_DEBUG_SIGAGG_ON) return true;
  if (debug_flags & BLS_DEBUG_SIGAGG_OFF) return false;
  if (k.sigagg >= 0) return k.sigagg != 0;
  return n >= SIGAGG_MIN_SETS && (n > PERSET_MAX_CALL || in_flight > k.perset_max_inflight);
}

// Group testing of a failed chunk's requests (instead of one final exponentiation per
// request, worker.ts:91-98).  Each request's product F_t (its sets' f and, on the
// aggregated path, its own signature-sum pairing) is left by k_indiv_coop; a test is
// FE(prod of a group's F_t) == 1 (k_group_coop), the same random-scalar batch check the
// reference runs over a chunk.  With the chunk's requests of status OK indexed 0 .. m-1:
//   pass A: the group of all of them (A), and for each bit j of the index the group G_j
//           of those with bit j set; each G_j's final exponentiation is also compared with
//           A's (k_group_cmp): FE(G_j) FE(rest_j) = FE(A), so FE(rest_j) == 1 iff
//           FE(G_j) == FE(A) -- every test answers for its complement too;
//   a single invalid request b fails exactly one of G_j, rest_j for every j (G_j where
//   b's bit j is set), which names b, and every other request sits in a passing test;
//   pass C: any other outcome (both of some G_j, rest_j failing: two or more invalid; an
//           index past m): every request alone.
// With one invalid request in a chunk of 16 that is 5 final exponentiations in one round
// instead of 16 (round 6; before it, without the comparison, pass B tested {b} alone and
// the rest together: 6 in two rounds, $BLS_GROUP_EQ=0 restores that); verdicts and the worker counters are the reference's (a test that passes is the
// batch the reference's retry would have passed request by request, with the same
// soundness).  On for chunks of >= 4 requests since round 6: once the failed chunks'
// requests stopped re-running their sets' own Miller loops and the chunks of a failing
// stream are checked without the merged check first, the saved final exponentiations
// outweigh the extra rounds -- cfg4 per-set requests 1.35M -> 1.50M sets/s steady, cfg5
// level (profiles/r06_ab_group_test.json; in rounds 4-5 it lost or was level,
// r04_ab_group_test.json, r05_ab_group_test_again.json).  $BLS_GROUP_TEST_MIN sets the
// smallest chunk tested so (0 = off); BLS_DEBUG_GROUP_TEST forces chunks of >= 4.
inline uint32_t group_test_min(const Knobs& k, uint32_t debug_flags) {
  return (debug_flags & BLS_DEBUG_GROUP_TEST) ? 4u : k.group_test_min;
}

// group sums (VerifyPass::group_sums) for a pass with at least $BLS_GROUP_SUMS_MIN (512)
// group-tested requests; 0 = always, $BLS_GROUP_SUMS=0 = never (SIZE_MAX).  They save Miller loops
// (cfg4 per-set requests, ~1,300 group-tested requests a pass: 1.52M -> 1.56M sets/s
// steady) but put a sum + Miller-loop stage in front of each round of tests, where the
// per-request sums ride in the requests' Miller-loop launch: with a few failed chunks
// a pass (the cfg5 slice, ~80 requests) that latency costs more (3.29M -> 3.05M)
// (profiles/r06_ab_group_sums.json)
inline size_t group_sums_min(const Knobs& k) { return k.group_sums ? (size_t)k.group_sums_min : SIZE_MAX; }

// Knobs::group_eq: complement inference in the group tests (verify_groups): pass A carries
// each chunk's test of all its requests and compares the bit groups' final exponentiations
// with it, so one invalid request is found without pass B ({b} alone, the rest together);
// the whole's value is the failed chunk check's own final exponentiation where that ran
// over the same requests (k_chunk_coop keeps it in b.chunk_fe), else a test of them.
// $BLS_GROUP_EQ=0 restores the two rounds, =2 always tests the whole

// Pippenger merged signature sum (k_msm) instead of the per-set [r] sig chains (k_chain
// role 2, ~1.6k Fp products per set) and the k_gsum levels: ~10 % fewer instructions per
// set, but its serial stages (segments, buckets, the windows' dependent additions) make
// the pass ~5 ms longer.  So it pays only when the device is VALU-bound with many sets in
// flight: 3.46M vs 3.21M sets/s at 16 x 16, level at 12 x 16, 1.89M vs 2.25M at 4 x 16
// (profiles/r03_ab_msm.json, round 3).  On the round-5 build it is level at 4 x 16 and
// ahead from 6 x 16 on (8 x 16: 3.24M / 3.30M vs 3.00M, profiles/r05_ab_msm_min.json), so
// by default on while the process has more than $BLS_MSM_MIN (60,000) sets in flight and
// the context's last pass passed its merged check (a failing pass needs the per-set chains
// after all: relaunching them cost the epoch slice with invalid sets 2.42M -> 2.1M sets/s);
// $BLS_MSM=1 / 0 forces it on / off.
inline bool msm_on(const Knobs& k, uint64_t in_flight) { return k.msm >= 0 ? k.msm == 1 : in_flight > k.msm_min; }

// Knobs::msm_overlap: the overlapped form of the Pippenger sum: its segment, bucket, window
// and final stages as roles of the first pass's Miller-loop launches (kernels/k_mlq.hip
// launch_k_mlqf_msm) instead of three launches in front of them.  On unless
// $BLS_MSM_OVERLAP=0 or the context's BLS_DEBUG_MSM_SERIAL; a pass whose f side is no
// k_mlf<1> of 1, 2 or 4 items per lane (MLF_PAIR, a forced cooperative packing) keeps the
// serial form either way.
//
// Knobs::ml_shared: shared Miller loops in k_mln (PipeBufs::ml_dom): on unless $BLS_ML_SHARED=0
//
// Knobs::sig_total: merged signature sum (with the merged check): one signature Miller
// loop per device pass instead of one per chunk; on unless $BLS_SIG_TOTAL=0
//
// Knobs::merged_skip_after_fail: after a pass whose merged check failed, a context's next
// pass skips it and checks its chunks straight away (each chunk's own signature sum paired
// in the pass's Miller-loop launch, then the per-chunk final exponentiations): a stream
// with invalid sets in most passes (the cfg4 per-set requests, the cfg5 epoch slice)
// otherwise pays the merged final exponentiation, then the chunk sums, their Miller loops
// and the chunk checks one after another on the failing call's path.  The first pass whose
// chunks all pass turns the merged check back on.  $BLS_MERGED_AFTER_FAIL=1 keeps it on
// every pass.

// How the verify path's host thread waits for its stream.  hipStreamSynchronize spins
// (so does hipEventSynchronize on a hipEventBlockingSync event in this runtime): with 16
// contexts each waiting through a ~95 ms pass the process held ~15.7 CPUs and the job's
// 16-CPU quota throttled it (profiles/r06_ab_sync_wait.json) -- CPU a beacon node's main
// thread and its other work need.  A pass of more than 2,048 sets (only the aggregated
// path takes those; tens of ms) polls an event with 50 us sleeps instead; smaller calls
// keep the spin: they can take the per-set path, a few ms, where polling at 1024-set
// calls cost 4 x 1 calls 7.2 -> 7.8 ms.  $BLS_SYNC=spin / poll forces either.
#define WAIT_POLL_MIN_SETS 2048u
inline bool wait_blocks(const Knobs& k, uint32_t n_sets) {
  return k.sync == 2 || (k.sync == 0 && n_sets > WAIT_POLL_MIN_SETS);
}

// Items per k_mlf lane for a launch now (kernels/k_mlq.hip launch_k_mlqf): 2 shares f's
// squarings between two pairs (fewer instructions:
// the rate when the device is VALU-bound), 1 halves the f chain (the rate when few sets
// are in flight and the pass latency sets it): 2.22M vs 2.00M sets/s with 64k sets in
// flight, 2.76M vs 2.90M with 128k (profiles/r03_ab_mlq_mlf.json).  By default the
// process's sets in flight (every context's verify call, bls_sets_in_flight) pick:
// 2 above $BLS_MLF_PL2_MIN (default 98,304) sets, 4 above $BLS_MLF_PL4_MIN (200,000:
// 3.55M vs 3.41M sets/s at 12 x 22), else 1.  $BLS_MLF_PER_LANE = 1, 2, 4 or 3 (MLF_PAIR)
// fixes it.  (Four items sharing f per lane PAIR, the squarings and line products split
// over the pair, lost 6-11 %: spills and ~9 % more lane work, profiles/r06_ab_mlf_pair4.json.)
// Up to $BLS_MLF_PAIR_MAX (16,384) sets in flight: two lanes per item (k_mlf2, MLF_PAIR;
// at two waves per SIMD, $BLS_MLF2_WAVES=1 for one): a solo pass's f side 4.7 vs 7.1 ms
// at 8,192 sets, 5.2 vs 7.2 ms at 16,384, but 8.8 vs 7.4 ms at 32,768
// (profiles/r04_ab_mlf_pair.json).
inline uint32_t mlf_per_lane(const Knobs& k, uint64_t in_flight) {
  if (k.mlf_per_lane) return k.mlf_per_lane;
  return in_flight > k.mlf_pl4_min ? 4u : (in_flight > k.mlf_pl2_min ? 2u : (in_flight > k.mlf_pair_max ? 1u : MLF_PAIR));
}

// Items per k_mlf lane for the launches after the first pass (a failed merged check's
// chunk signature sums, the individually verified requests' own loops and sums): their
// items never share f, so more than one per lane only lengthens the chain that the failing
// call waits on (4 per lane ran each such launch for the whole 14 ms of a plateau pass's f
// side, profiles/r05_cfg5_fallback.json).  Two lanes per item up to $BLS_MLF_PAIR_MAX
// items, else one; $BLS_MLF_PER_LANE still fixes it; $BLS_MLF_ALONE=0 returns 0 (the
// launches keep the first pass's shape, as before round 5's change).
inline uint32_t mlf_per_lane_alone(const Knobs& k, uint32_t count) {
  if (!k.mlf_alone) return 0u;
  if (k.mlf_per_lane) return k.mlf_per_lane;
  return count <= k.mlf_pair_max ? MLF_PAIR : 1u;
}

// Sets per wavefront for a batch: 1 for small batches (latency: one set per two
// wavefronts spreads a small call over more SIMDs); from BLS_PACK_MIN_SETS sets on, 2
// while the process has at most $BLS_PACK3_INFLIGHT (2,048) sets in flight, else 3
// (three sets' steps share one wavefront's lanes: on the round-5 interpreter 1024-set
// calls at 4 x 1 / 8 x 1 / 12 x 1 contexts run 0.58M / 0.70M / 0.79M sets/s packed 3
// against 0.49-0.53M / 0.63-0.66M / 0.68-0.70M packed 2 and ~0.26M unpacked, but at
// 2 x 1 0.32M against 0.35M; profiles/r05_ab_perset_pack.json; round 4 had 2 ahead of 3
// everywhere).  $BLS_PACK (1, 2 or 3) forces a packing; $BLS_PACK_MIN overrides the
// threshold.
inline uint32_t pack_for(const Knobs& k, uint32_t n_sets, uint64_t in_flight) {
  if (k.pack) return k.pack;
  if (n_sets < k.pack_min) return 1u;
  return in_flight > k.pack3_inflight ? 3u : 2u;
}

}  // namespace bls
