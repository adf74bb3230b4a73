// Host-side planning of a verify pass: pure index arithmetic over the caller's offsets,
// no HIP, no context, no environment.  bls_gpu.hip stages what these functions return and
// the kernels index memory through it, so each plan is also checked on the CPU
// (tests/native/plan_exports.hpp, tests/test_plan_cpu.py, and under sanitizers
// tests/native/plan_host.cpp).  Whatever selects a variant comes in as a parameter; at the
// end plan_pass, the decision table of a whole pass, takes the parsed knobs (bls/knobs.hpp)
// the same way.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../../include/lodestar_bls.h"
#include "knobs.hpp"
#include "plan_shape.hpp"

namespace bls {

// ---- the caller's batch ---------------------------------------------------------------

// Shape checks of one caller batch: 0, or -2 with the reason in err.  The kernels and the
// verify_many join index sets and key lists through these offsets, so they must start at
// 0, be monotone and end at the array sizes.
inline int check_batch(const bls_batch* in, const char* what, char* err, size_t err_len) {
  const uint32_t n = in->n_sets, R = in->n_reqs;
  if (R == 0) return 0;
  if (!in->req_set_offsets) {
    snprintf(err, err_len, "%s: req_set_offsets missing", what);
    return -2;
  }
  if (in->req_set_offsets[0] != 0 || in->req_set_offsets[R] != n) {
    snprintf(err, err_len, "%s: req_set_offsets must run from 0 to n_sets", what);
    return -2;
  }
  if (in->set_pk_offsets == nullptr && in->pubkeys == nullptr && n > 0) {
    snprintf(err, err_len, "%s: no pubkeys given", what);
    return -2;
  }
  if (n > 0 && (!in->messages || !in->signatures)) {
    snprintf(err, err_len, "%s: messages / signatures missing", what);
    return -2;
  }
  for (uint32_t r = 0; r < R; ++r) {
    if (in->req_set_offsets[r] > in->req_set_offsets[r + 1]) {
      snprintf(err, err_len, "%s: req_set_offsets not monotone at %u", what, r);
      return -2;
    }
  }
  if (in->set_pk_offsets) {
    if (in->set_pk_offsets[0] != 0) {
      snprintf(err, err_len, "%s: set_pk_offsets[0] != 0", what);
      return -2;
    }
    for (uint32_t i = 0; i < n; ++i) {
      if (in->set_pk_offsets[i] > in->set_pk_offsets[i + 1]) {
        snprintf(err, err_len, "%s: set_pk_offsets not monotone at %u", what, i);
        return -2;
      }
    }
    if (in->set_pk_offsets[n] > 0 && !in->pk_indices) {
      snprintf(err, err_len, "%s: pk_indices missing", what);
      return -2;
    }
  }
  return 0;
}

// chunkifyMaximizeChunkSize (beacon-node/src/chain/bls/multithread/utils.ts:4-19)
inline void chunkify_maximize_chunk_size(uint32_t n, uint32_t min_per_chunk, std::vector<uint32_t>& bounds) {
  bounds.clear();
  uint32_t chunk_count = n / min_per_chunk;
  bounds.push_back(0);
  if (chunk_count <= 1) {
    bounds.push_back(n);
    return;
  }
  uint32_t per = (n + chunk_count - 1) / chunk_count;
  for (uint32_t i = per; i < n; i += per) bounds.push_back(i);
  bounds.push_back(n);
}

// Host-side plan of one verify call: chunks over the batchable requests
// (BATCHABLE_MIN_PER_CHUNK = 16, worker.ts:17,56) and the non-batchable list.
struct BatchPlan {
  std::vector<uint32_t> chunk_off, chunk_reqs, nonbatch_reqs;
};

inline void plan_batch(const bls_batch* in, BatchPlan& p) {
  std::vector<uint32_t> batchable;
  p.nonbatch_reqs.clear();
  for (uint32_t r = 0; r < in->n_reqs; ++r) {
    if (in->req_batchable && in->req_batchable[r]) batchable.push_back(r);
    else p.nonbatch_reqs.push_back(r);
  }
  p.chunk_off.clear();
  p.chunk_reqs = batchable;
  if (batchable.empty()) {
    p.chunk_off.push_back(0);
    return;
  }
  chunkify_maximize_chunk_size((uint32_t)batchable.size(), 16, p.chunk_off);
}

// plan_batch over several worker messages submitted together (bls_gpu_verify_many):
// each message's batchable requests are chunked on their own (worker.ts:56 runs per
// message), so the chunks never straddle a message; req_bounds[k] = first request of
// message k, req_bounds[n_msgs] = n_reqs.
inline void plan_batch_msgs(const bls_batch* in, const std::vector<uint32_t>& req_bounds, BatchPlan& p) {
  p.chunk_off.assign(1, 0);
  p.chunk_reqs.clear();
  p.nonbatch_reqs.clear();
  std::vector<uint32_t> batchable, bounds;
  for (size_t m = 0; m + 1 < req_bounds.size(); ++m) {
    batchable.clear();
    for (uint32_t r = req_bounds[m]; r < req_bounds[m + 1]; ++r) {
      if (in->req_batchable && in->req_batchable[r]) batchable.push_back(r);
      else p.nonbatch_reqs.push_back(r);
    }
    if (batchable.empty()) continue;
    chunkify_maximize_chunk_size((uint32_t)batchable.size(), 16, bounds);
    const uint32_t base = (uint32_t)p.chunk_reqs.size();
    p.chunk_reqs.insert(p.chunk_reqs.end(), batchable.begin(), batchable.end());
    for (size_t k = 1; k < bounds.size(); ++k) p.chunk_off.push_back(base + bounds[k]);
  }
}

// Plan of one bls_gpu_verify_same_message call over the verify pass: every set is a
// one-set batchable request (request index == set index, so a failing job's fallback gives
// the one-set path's verdicts), every job of >= 2 sets is a caller-defined chunk -- ONE
// random-scalar batch whatever its size, not chunked at 16 -- and a 1-set job is a request
// verified on its own directly.
struct SameMsgPlan {
  BatchPlan plan;
};

// shape checks of the caller's batch: nullptr, or what is wrong (the call returns -2)
inline const char* check_same_message(const bls_same_msg_batch* in, const int32_t* set_verdicts) {
  if (!in->job_set_offsets || !in->messages || !in->pk_indices || !in->signatures || !set_verdicts)
    return "a required pointer is NULL";
  if (in->job_set_offsets[0] != 0 || in->job_set_offsets[in->n_jobs] != in->n_sets)
    return "job_set_offsets must run from 0 to n_sets";
  for (uint32_t j = 0; j < in->n_jobs; ++j) {
    const uint32_t beg = in->job_set_offsets[j], end = in->job_set_offsets[j + 1];
    if (end <= beg || end > in->n_sets) return "empty job or offsets not monotone";
    if (end - beg > BLS_SAME_MSG_MAX_JOB) return "job of more than BLS_SAME_MSG_MAX_JOB sets";
  }
  return nullptr;
}

inline void plan_same_message(const bls_same_msg_batch* in, SameMsgPlan& p) {
  p.plan.chunk_off.assign(1, 0);
  p.plan.chunk_reqs.clear();
  p.plan.nonbatch_reqs.clear();
  for (uint32_t j = 0; j < in->n_jobs; ++j) {
    const uint32_t beg = in->job_set_offsets[j], end = in->job_set_offsets[j + 1];
    if (end - beg == 1) {
      p.plan.nonbatch_reqs.push_back(beg);
      continue;
    }
    for (uint32_t i = beg; i < end; ++i) p.plan.chunk_reqs.push_back(i);
    p.plan.chunk_off.push_back((uint32_t)p.plan.chunk_reqs.size());
  }
}

// Plan of one bls_gpu_verify_deposits call over the verify pass: every deposit is a one-set
// batchable request (request index == deposit index), chunked like any batchable request
// (plan_batch: chunkifyMaximizeChunkSize at 16).  The batch carries the signatures only:
// the pass's front kernel makes each request's key and signing root on the device from the
// deposit's fields, so there is nothing to dedup and no key list.
struct DepositPlan {
  std::vector<uint32_t> off;       // n + 1: 0, 1, .., n (request r owns set r)
  std::vector<uint8_t> batchable;  // n ones
};

// shape checks of the caller's batch: nullptr, or what is wrong (the call returns -2)
inline const char* check_deposits(const bls_deposit_batch* in, const int32_t* verdicts) {
  if (in->n > BLS_DEPOSITS_MAX_CALL) return "more than BLS_DEPOSITS_MAX_CALL deposits";
  if (!in->pubkeys48 || !in->withdrawal_credentials || !in->amounts || !in->signatures || !in->domain || !verdicts)
    return "a required pointer is NULL";
  return nullptr;
}

// fills p and points `all` at it (p must outlive the pass)
inline void plan_deposits(const bls_deposit_batch* in, DepositPlan& p, bls_batch& all) {
  const uint32_t n = in->n;
  p.off.resize((size_t)n + 1);
  for (uint32_t i = 0; i <= n; ++i) p.off[i] = i;
  p.batchable.assign(n, 1);
  memset(&all, 0, sizeof(all));
  all.n_sets = n;
  all.n_reqs = n;
  all.req_set_offsets = p.off.data();
  all.req_batchable = p.batchable.data();
  all.signatures = in->signatures;
  all.seed = in->seed;
}

// Signing-root dedup for stage_pre: uniq = the first set of each distinct 32-byte
// root (in set order), rep[i] = that first set for set i.  Committee-shared roots
// (~512 attesters per root) then pay hash_to_field + SSWU once.
// Open addressing over a mix of all 32 bytes, so crafted roots cost probes, not
// wrong answers.  Returns the number of distinct roots.
inline uint32_t plan_msg_dedup(const uint8_t* msgs, uint32_t n, std::vector<uint32_t>& uniq,
                               std::vector<uint32_t>& rep) {
  uniq.clear();
  rep.resize(n);
  uint32_t cap = 16;
  while (cap < 2 * n) cap <<= 1;
  std::vector<uint32_t> slot(cap, 0xffffffffu);
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t* m = msgs + 32ull * i;
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (int w = 0; w < 4; ++w) {
      uint64_t v;
      memcpy(&v, m + 8 * w, 8);
      h = (h ^ v) * 0xff51afd7ed558ccdull;
      h ^= h >> 32;
    }
    uint32_t pos = (uint32_t)h & (cap - 1);
    for (;;) {
      const uint32_t j = slot[pos];
      if (j == 0xffffffffu) {
        slot[pos] = i;
        rep[i] = i;
        uniq.push_back(i);
        break;
      }
      if (memcmp(msgs + 32ull * j, m, 32) == 0) {
        rep[i] = j;
        break;
      }
      pos = (pos + 1) & (cap - 1);
    }
  }
  return (uint32_t)uniq.size();
}

// ---- group sums (k_gsum / k_gsum1) ------------------------------------------------------

// Segmented-sum plan over groups of sets: the groups' set indices (group-major) and, per
// level, (beg, end) segments of at most GSUM_FAN items that never straddle a group;
// level 0 indexes gsets, level L > 0 the outputs of level L - 1.  After the last level
// there is one point per group, in group order.
struct GsumPlan {
  std::vector<uint32_t> gsets;
  std::vector<uint32_t> seg;        // every level's pairs, concatenated
  std::vector<uint32_t> level_off;  // level L: pairs [level_off[L], level_off[L + 1])
};

// groups given as explicit set lists: group g = sets[goff[g] .. goff[g + 1])
inline void plan_gsum_sets(const std::vector<uint32_t>& goff, const std::vector<uint32_t>& sets, GsumPlan& p) {
  p.gsets = sets;
  p.seg.clear();
  p.level_off.assign(1, 0);
  const size_t G = goff.size() - 1;
  std::vector<uint32_t> cnt(G);
  for (size_t g = 0; g < G; ++g) {
    const uint32_t gb = goff[g], ge = goff[g + 1];
    cnt[g] = 0;
    for (uint32_t k = gb; k < ge || (k == gb && gb == ge); k += GSUM_FAN) {
      p.seg.push_back(k);
      p.seg.push_back(k + GSUM_FAN < ge ? k + GSUM_FAN : ge);
      ++cnt[g];
      if (gb == ge) break;
    }
  }
  p.level_off.push_back((uint32_t)(p.seg.size() / 2));
  for (;;) {
    bool more = false;
    for (uint32_t c : cnt) more = more || c > 1;
    if (!more) break;
    uint32_t pos = 0;
    for (size_t g = 0; g < G; ++g) {
      const uint32_t c = cnt[g];
      uint32_t nc = 0;
      for (uint32_t k = 0; k < c; k += GSUM_FAN, ++nc) {
        p.seg.push_back(pos + k);
        p.seg.push_back(pos + (k + GSUM_FAN < c ? k + GSUM_FAN : c));
      }
      pos += c;
      cnt[g] = nc;
    }
    p.level_off.push_back((uint32_t)(p.seg.size() / 2));
  }
}

// groups of requests (chunks, individually verified requests): their sets in order
inline void plan_gsum(const uint32_t* req_off, const std::vector<uint32_t>& grp_off,
                      const std::vector<uint32_t>& grp_reqs, GsumPlan& p) {
  std::vector<uint32_t> goff(1, 0), sets;
  for (size_t g = 0; g + 1 < grp_off.size(); ++g) {
    for (uint32_t k = grp_off[g]; k < grp_off[g + 1]; ++k) {
      const uint32_t r = grp_reqs[k];
      for (uint32_t i = req_off[r]; i < req_off[r + 1]; ++i) sets.push_back(i);
    }
    goff.push_back((uint32_t)sets.size());
  }
  plan_gsum_sets(goff, sets, p);
}

// The workspace a pass of n sets and R requests keeps for any plan over disjoint sets in
// at most R groups: gseg_cap uint32s for every level's pairs (fan-in >= 4), gtmp_cap
// points per buffer for the level-0 outputs, n set indices.
inline size_t gseg_cap(uint32_t n, uint32_t R) { return 2ull * (n / 2 + 12ull * R + 8); }
inline size_t gtmp_cap(uint32_t n, uint32_t R) { return (size_t)n / GSUM_FAN + R + 1; }
inline bool gsum_fits(const GsumPlan& p, uint32_t n, uint32_t R) {
  return p.gsets.size() <= n && p.seg.size() <= gseg_cap(n, R) &&
         (p.level_off.size() < 2 || p.level_off[1] <= gtmp_cap(n, R));
}

// ---- Miller-loop units and product domains ----------------------------------------------

// Miller-loop units (sum r_i pk_i per root): within each chunk, the sets
// signing the same root (msg_rep: the root's first set) form one unit, paired once as
// ML(sum r_i pk_i, H(root)).  Used when it at least halves the chunks' Miller loops.
struct UnitPlan {
  std::vector<uint32_t> set_unit, unit_rep, unit_off, goff, members;
  uint32_t n_units = 0;
};

inline bool plan_units(const uint32_t* req_off, const BatchPlan& plan, const std::vector<uint32_t>& msg_rep,
                       uint32_t n, UnitPlan& u) {
  const uint32_t C = (uint32_t)plan.chunk_off.size() - 1;
  if (msg_rep.empty() || C == 0) return false;
  u.set_unit.assign(n, UNIT_NONE);
  u.unit_off.assign(1, 0);
  std::vector<uint32_t> stamp(n, 0xFFFFFFFFu), unit_of(n, 0);
  std::vector<std::vector<uint32_t>> mem;
  uint32_t in_chunks = 0;
  for (uint32_t c = 0; c < C; ++c) {
    for (uint32_t k = plan.chunk_off[c]; k < plan.chunk_off[c + 1]; ++k) {
      const uint32_t r = plan.chunk_reqs[k];
      for (uint32_t i = req_off[r]; i < req_off[r + 1]; ++i) {
        const uint32_t rep = msg_rep[i];
        if (stamp[rep] != c) {
          stamp[rep] = c;
          unit_of[rep] = (uint32_t)mem.size();
          mem.emplace_back();
          u.unit_rep.push_back(rep);
        }
        u.set_unit[i] = unit_of[rep];
        mem[unit_of[rep]].push_back(i);
        ++in_chunks;
      }
    }
    u.unit_off.push_back((uint32_t)mem.size());
  }
  u.n_units = (uint32_t)mem.size();
  if (2ull * u.n_units > in_chunks) return false;
  u.goff.assign(1, 0);
  u.members.clear();
  for (auto& m : mem) {
    u.members.insert(u.members.end(), m.begin(), m.end());
    u.goff.push_back((uint32_t)u.members.size());
  }
  return true;
}

// The Miller-loop units of a same-message call (plan_same_message): unit c = all the sets
// of chunk c, paired once as e(sum r_i pk_i, H(root)); rep = the set that computed the
// root's H (plan_msg_dedup's first set of the root; without dedup the job's own first set)
inline void units_same_message(const BatchPlan& plan, const std::vector<uint32_t>& msg_rep, uint32_t n, UnitPlan& u) {
  const uint32_t C = (uint32_t)plan.chunk_off.size() - 1;
  u.set_unit.assign(n, UNIT_NONE);
  u.unit_off.resize(C + 1);
  u.unit_rep.resize(C);
  u.goff = plan.chunk_off;
  u.members = plan.chunk_reqs;  // (every request is one set: request index == set index)
  for (uint32_t c = 0; c < C; ++c) {
    u.unit_off[c] = c;
    const uint32_t first = plan.chunk_reqs[plan.chunk_off[c]];
    u.unit_rep[c] = msg_rep.empty() ? first : msg_rep[first];
    for (uint32_t k = plan.chunk_off[c]; k < plan.chunk_off[c + 1]; ++k) u.set_unit[plan.chunk_reqs[k]] = c;
  }
  u.unit_off[C] = C;
  u.n_units = C;
}

// Product domain of every first-pass Miller-loop item -- sets [0, n), chunk signature sums
// [n, n + C), units [n + C, n + C + U) (units: nullptr = none) -- for PipeBufs::ml_dom:
// its chunk, 0x80000000 | request for a non-batchable request's sets, 0xFFFFFFFF none.
inline void plan_ml_domains(const uint32_t* req_off, const BatchPlan& plan, const UnitPlan* units, uint32_t n,
                            std::vector<uint32_t>& dom) {
  const uint32_t C = (uint32_t)plan.chunk_off.size() - 1, unit_base = n + C;
  dom.assign((size_t)unit_base + (units ? units->n_units : 0u), 0xFFFFFFFFu);
  for (uint32_t ch = 0; ch < C; ++ch) {
    for (uint32_t k = plan.chunk_off[ch]; k < plan.chunk_off[ch + 1]; ++k) {
      const uint32_t r = plan.chunk_reqs[k];
      for (uint32_t i = req_off[r]; i < req_off[r + 1]; ++i) dom[i] = ch;
    }
    dom[n + ch] = ch;
    if (units)
      for (uint32_t u = units->unit_off[ch]; u < units->unit_off[ch + 1]; ++u) dom[unit_base + u] = ch;
  }
  for (uint32_t r : plan.nonbatch_reqs)
    for (uint32_t i = req_off[r]; i < req_off[r + 1]; ++i) dom[i] = 0x80000000u | r;
}

// ---- the individually verified requests -------------------------------------------------

struct GtChunk {
  uint32_t beg, end;  // its requests in the indiv list
  uint32_t ch;        // its chunk (b.chunk_fe)
};

// Requests verified on their own: the non-batchable ones, then the failed chunks'
// (worker.ts:91-98).  A failed chunk of >= gt_min requests is group-tested instead of
// paying one final exponentiation per request; its requests follow the directly verified
// ones (reqs[0, n_direct)) in the list.
struct IndivPlan {
  std::vector<uint32_t> reqs;
  std::vector<GtChunk> gt_chunks;
  uint32_t n_direct = 0;
};

inline void plan_indiv(const BatchPlan& plan, const int32_t* chunk_ok, uint32_t gt_min, IndivPlan& p) {
  const uint32_t C = (uint32_t)plan.chunk_off.size() - 1;
  p.reqs = plan.nonbatch_reqs;
  p.gt_chunks.clear();
  for (int pass = 0; pass < 2; ++pass)
    for (uint32_t ch = 0; ch < C; ++ch) {
      if (chunk_ok[ch] == 1) continue;
      const uint32_t m = plan.chunk_off[ch + 1] - plan.chunk_off[ch];
      if ((m >= gt_min) != (pass == 1)) continue;
      const uint32_t beg = (uint32_t)p.reqs.size();
      for (uint32_t k = plan.chunk_off[ch]; k < plan.chunk_off[ch + 1]; ++k) p.reqs.push_back(plan.chunk_reqs[k]);
      if (pass == 1) p.gt_chunks.push_back({beg, (uint32_t)p.reqs.size(), ch});
    }
  p.n_direct = p.gt_chunks.empty() ? (uint32_t)p.reqs.size() : p.gt_chunks.front().beg;
}

// The sets of reqs[first_t, ..) (the failed chunks' requests) that run their own Miller
// loop again: all of them, or only those paired in a unit (set_unit, nullable).
inline void plan_own_sets(const uint32_t* req_off, const std::vector<uint32_t>& reqs, size_t first_t, bool all,
                          const uint32_t* set_unit, std::vector<uint32_t>& own) {
  own.clear();
  for (size_t t = first_t; t < reqs.size(); ++t)
    for (uint32_t i = req_off[reqs[t]]; i < req_off[reqs[t] + 1]; ++i)
      if (all || (set_unit && set_unit[i] != UNIT_NONE)) own.push_back(i);
}

// ... as (first set, count) runs of consecutive sets, one launch each (a failed chunk's
// requests are adjacent)
inline void plan_own_runs(const uint32_t* req_off, const std::vector<uint32_t>& reqs, size_t first_t,
                          std::vector<uint32_t>& runs) {
  runs.clear();
  uint32_t run_beg = 0, run_end = 0;
  for (size_t t = first_t; t <= reqs.size(); ++t) {
    const bool last = t == reqs.size();
    const uint32_t beg = last ? 0 : req_off[reqs[t]], end = last ? 0 : req_off[reqs[t] + 1];
    if (!last && run_end > run_beg && beg == run_end) {
      run_end = end;
      continue;
    }
    if (run_end > run_beg) {
      runs.push_back(run_beg);
      runs.push_back(run_end - run_beg);
    }
    run_beg = beg;
    run_end = end;
  }
}

// k_fold groups of the requests' f: [beg, end) pairs of at most BLS_FOLD1 consecutive sets
// (groups[0, 2 n_fold1)), then, for every span of BLS_FOLD sets holding more than one of
// those, the span (the first-level products are multiplied BLS_FOLD / BLS_FOLD1 at a time)
struct FoldPlan {
  std::vector<uint32_t> groups;
  uint32_t n_fold1 = 0;
  bool any_fold = false;  // some group has more than one set
};

inline void plan_fold_groups(const uint32_t* req_off, const std::vector<uint32_t>& reqs, FoldPlan& f) {
  f.groups.clear();
  f.any_fold = false;
  for (uint32_t r : reqs) {
    const uint32_t beg = req_off[r], end = req_off[r + 1];
    for (uint32_t g = beg; g < end; g += BLS_FOLD1) {
      const uint32_t ge = g + BLS_FOLD1 < end ? g + BLS_FOLD1 : end;
      f.groups.push_back(g);
      f.groups.push_back(ge);
      f.any_fold = f.any_fold || ge - g > 1;
    }
  }
  f.n_fold1 = (uint32_t)(f.groups.size() / 2);
  for (uint32_t r : reqs) {
    const uint32_t beg = req_off[r], end = req_off[r + 1];
    for (uint32_t g = beg; g < end; g += BLS_FOLD) {
      const uint32_t ge = g + BLS_FOLD < end ? g + BLS_FOLD : end;
      if (ge - g <= BLS_FOLD1) continue;  // one first-level group: already folded
      f.groups.push_back(g);
      f.groups.push_back(ge);
    }
  }
}

// ---- group tests (pass A) ---------------------------------------------------------------

// One group-tested chunk: its requests of status OK and where its tests sit in pass A
struct GroupTestChunk {
  std::vector<uint32_t> ok;  // indiv indices of the requests of status OK
  bool has_err = false;
  bool whole = false;        // a test of all of ok at `first` (else the chunk check's value)
  uint32_t first = 0, nbits = 0;
  int32_t b = -1;            // the one invalid request's position in ok (pass B), -1 none
};

// tests: test g = members[off[g], off[g + 1]) (indiv indices), compared with test ref[g]
struct GroupTestsA {
  std::vector<GroupTestChunk> cs;  // the chunks with a request of status OK
  std::vector<uint32_t> off, members, ref;
};

// Pass A of the group tests: per chunk, a test of all its requests of status OK (verdict
// == 2; others keep their -code) when one is needed, then for each bit j of their index
// the group of those with bit j set.  eq: complement inference is on (every bit group is
// compared with the whole); chunk_fe: the failed chunk checks' own final exponentiations
// were kept, so a chunk without an erroneous request takes the whole's value from there
// (ref = REF_CHUNK | chunk) instead of a test.
inline void plan_group_tests_a(const std::vector<GtChunk>& chunks, const int32_t* verdict, bool eq, bool chunk_fe,
                               GroupTestsA& a) {
  a.cs.clear();
  a.off.assign(1, 0);
  a.members.clear();
  a.ref.clear();
  auto add_test = [&](const std::vector<uint32_t>& m, uint32_t r) {
    a.members.insert(a.members.end(), m.begin(), m.end());
    a.off.push_back((uint32_t)a.members.size());
    a.ref.push_back(r);
  };
  for (const auto& ch : chunks) {
    GroupTestChunk c;
    for (uint32_t t = ch.beg; t < ch.end; ++t) {
      if (verdict[t] == 2) c.ok.push_back(t);
      else c.has_err = true;  // its -code stays
    }
    if (c.ok.empty()) continue;
    c.first = (uint32_t)a.off.size() - 1;
    // the whole's value: the failed chunk check's own final exponentiation when it ran
    // over exactly these requests (no erroneous one), else a test of them
    const bool from_check = eq && chunk_fe && !c.has_err && c.ok.size() > 1;
    c.whole = !from_check && (eq || c.has_err || c.ok.size() == 1);
    if (c.whole) add_test(c.ok, REF_NONE);
    const uint32_t m = (uint32_t)c.ok.size();
    while (m > 1 && (1u << c.nbits) < m) ++c.nbits;
    for (uint32_t j = 0; j < c.nbits; ++j) {
      std::vector<uint32_t> g;
      for (uint32_t k = 0; k < m; ++k)
        if ((k >> j) & 1u) g.push_back(c.ok[k]);
      add_test(g, from_check ? (REF_CHUNK | ch.ch) : c.first);
    }
    a.cs.push_back(std::move(c));
  }
}

// The group tests' workspace for R requests in C chunks (the passes reuse it): pass A <=
// 1 + 13 tests per chunk (chunks of < 8192 requests) of <= 8 m members in all, pass B 2
// tests per chunk, pass C one test per request
inline size_t grp_cap(uint32_t R, uint32_t C) { return (size_t)R + 14ull * C + 2; }
inline size_t grp_mem_cap(uint32_t R) { return 8ull * R + 16; }
inline bool group_tests_fit(const GroupTestsA& a, uint32_t R, uint32_t C) {
  return a.members.size() <= grp_mem_cap(R) && a.off.size() - 1 <= grp_cap(R, C);
}

// ---- the pass ---------------------------------------------------------------------------

// what the entry point asks of the pass ...
struct PassAsk {
  bool partial;            // the Miller-loop partial of one shard (bls_gpu_partial)
  const SameMsgPlan* sm;   // verify_same_message: its own plan
  bool dep;                // a deposit call: n one-set batchable requests, keys and roots made on the device
  const std::vector<uint32_t>* req_bounds;  // verify_many: the messages' first requests
};

// ... and what its context and process contribute
struct PassEnv {
  uint32_t debug_flags;     // bls_gpu_set_debug_flags
  bool last_merged_failed;  // the context's last pass failed its merged check
  uint64_t in_flight;       // sets in the verify calls now running in this process, this call's included
};

// Every decision and count of a pass, fixed by plan_pass before anything is staged.
struct PassShape {
  uint32_t n, R, n_chunks, n_uniq, n_pk_idx;
  bool partial, sm, dedup;
  bool dep;  // a deposit call (PassAsk::dep)
  // Merged check: with only batchable requests and >= 2 chunks, first test the product of
  // every f_i with ONE final exponentiation (k_fprod tree); it passes iff every chunk would
  // (the same random-scalar batch, just larger), so chunk_ok is all 1 and the per-chunk
  // final exponentiations are skipped.  A failing merged check (or a request with an error
  // status) falls back to k_chunk_coop, so verdicts and stats stay those of the chunked
  // worker (worker.ts:56-88).  merged_skipped: Knobs::merged_skip_after_fail.
  bool merged_eligible, merged_skipped, merged;
  // aggregated-signature path (a same-message call always: the per-set k_pset path would
  // bring back one Miller loop pair per set)
  bool sigagg;
  bool use_units;  // Miller-loop units; same-message jobs: one per job, whatever the flags
  bool smsum;      // ... and their sums of r_i pk_i and r_i sig_i by k_smsum, one wavefront per job
  // Merged signature sum: under the merged check the chunks' signature sums only ever meet
  // in the product of every f, and prod_c e(-g1, S_c) = e(-g1, sum_c S_c) after the final
  // exponentiation, so the first pass sums every chunk's r_i sig_i into ONE point (chunk
  // group 0; the other chunk groups are empty, so k_vset gives them f = 1) and pairs it
  // once.  A failing merged check re-sums per chunk and pairs each sum before the
  // per-chunk final exponentiations, so chunk verdicts are unchanged.  (Not for
  // same-message jobs: each job's sum is paired in the first pass's launch.)
  bool use_total;
  // ... and under it the sum is one Pippenger MSM over the live sets (kernels/k_msm.hip)
  // instead of per-set [r] sig chains + k_gsum levels; the per-set RS are made (k_chain
  // role 2 alone) only when the merged check fails and the chunks' own sums are needed
  // (an MSM entry packs its bucket slot in 22 bits and a bucket takes up to 2 entries per
  // set: passes above MSM_MAX_SETS keep the group sums)
  bool use_msm;
  bool msm_overlap;  // ... with its long stages inside the Miller-loop launches, if the f-side shape allows
  bool ml_shared;  // k_mln shares one loop among four consecutive live items of one domain
  // f / chain layout: sets [0, n) | chunk signature sums [n, n + C) | units
  // [n + C, n + C + U) | individual requests' signature sums [n + C + U, .. + R)
  uint32_t n_units, unit_base, indiv_vbase, n_total;
  uint32_t n_prod;  // the f's of every set, chunk group and unit: what the product trees multiply
  // group tests: the smallest chunk tested so, whether any chunk is that large (their
  // buffers are carved only then), $BLS_GROUP_EQ, the fewest group-tested requests that
  // take group sums (SIZE_MAX: never)
  uint32_t gt_min;
  bool gt_possible;
  int gt_eq_mode;
  size_t gsums_min;
  // SIMT final exponentiations (kernels/k_fin_simt.hip) for a failing pass's many chunk
  // checks / requests verified alone: 4 Fp12 per task, carved when a pass could need them.
  // fe_min: the task count from which they run one lane per task ($BLS_FE_SIMT_MIN;
  // default 0 = off: at 256 the cfg4 per-set-request slice ran 1.04M vs 1.15M sets/s steady
  // and the cfg5 slice 2.56M vs 2.83M -- a lane's ~8k dependent Fp products take ~8 ms, and
  // those passes wait on the tail's latency, not on device time; profiles/r06_ab_fe_simt.json)
  uint32_t fe_min;
  bool fe_simt_possible;
  uint32_t init_set_flag, pack, mlf_pl;  // BLS_DEBUG_FORCE_EXACT, _PACK, _MLF_PL
  bool pl_forced;                        // a test forces the items per k_mlf lane
  bool merged_after_fail;                // the context's last pass failed its merged check
  size_t gseg_cap, gtmp_cap, grp_cap, grp_mem_cap;
};

// the host vectors a pass stages with its inputs
struct PassPlans {
  BatchPlan built;  // unless the caller brought its own (same-message calls)
  const BatchPlan* plan;
  std::vector<uint32_t> msg_uniq, msg_rep;
  UnitPlan units;
  GsumPlan chunk_gsum, unit_gsum, total_gsum;
  std::vector<uint32_t> ml_dom;
  std::vector<uint32_t> agg_list;  // aggregate sets big enough for a wavefront each (k_pk_agg)
};

// The decision table of a pass: from what the call asks, what its context contributes and
// the process's knobs (bls/knobs.hpp) it fills the plans and returns the shape.  Nothing
// else reads a debug flag, a knob that shapes the pass or the merged-check history.
inline PassShape plan_pass(const bls_batch* in, const PassAsk& a, const PassEnv& env, const Knobs& k,
                           PassPlans& pl) {
  PassShape sh;
  memset(&sh, 0, sizeof(sh));
  const uint32_t flags = env.debug_flags;
  const uint32_t n = sh.n = in->n_sets, R = sh.R = in->n_reqs;
  const uint32_t* req_off = in->req_set_offsets;
  sh.partial = a.partial;
  sh.sm = a.sm != nullptr;
  sh.dep = a.dep;
  if (a.sm) {
    pl.plan = &a.sm->plan;  // every job a caller-defined chunk (plan_same_message)
  } else {
    if (a.req_bounds) plan_batch_msgs(in, *a.req_bounds, pl.built);
    else plan_batch(in, pl.built);
    pl.plan = &pl.built;
  }
  const BatchPlan& plan = *pl.plan;
  // (a deposit call's roots are made on the device: nothing to dedup on the host)
  const bool no_dedup = sh.dep || (flags & BLS_DEBUG_NO_MSG_DEDUP);
  sh.n_uniq = no_dedup ? n : plan_msg_dedup(in->messages, n, pl.msg_uniq, pl.msg_rep);
  sh.dedup = sh.n_uniq < n;
  // (same-message and deposit calls neither read nor write the context's merged-check
  // history: invalid deposits are normal and must not shape the next gossip pass)
  sh.merged_after_fail = !sh.dep && env.last_merged_failed;
  sh.merged_eligible = !sh.partial && plan.chunk_off.size() > 2 && plan.nonbatch_reqs.empty() && n > 0 &&
                       !(flags & BLS_DEBUG_NO_MERGED_CHECK);
  sh.merged_skipped = sh.merged_eligible && !sh.sm && sh.merged_after_fail && k.merged_skip_after_fail &&
                      !(flags & BLS_DEBUG_MERGED_EVERY_PASS);
  sh.merged = sh.merged_eligible && !sh.merged_skipped;
  const uint32_t C = sh.n_chunks = (uint32_t)plan.chunk_off.size() - 1;
  sh.n_pk_idx = in->set_pk_offsets ? in->set_pk_offsets[n] : 0;
  sh.sigagg = n > 0 && (sh.sm || use_sigagg(k, flags, n, env.in_flight));
  if (sh.sm && C > 0) units_same_message(plan, pl.msg_rep, n, pl.units);
  sh.use_units = sh.sm ? C > 0
                       : sh.sigagg && sh.dedup && !(flags & BLS_DEBUG_NO_UNITS) &&
                             plan_units(req_off, plan, pl.msg_rep, n, pl.units);
  sh.smsum = sh.sm && sh.use_units;
  sh.n_units = sh.use_units ? pl.units.n_units : 0;
  sh.unit_base = n + C;
  sh.indiv_vbase = n + C + sh.n_units;
  sh.n_total = sh.sigagg ? sh.indiv_vbase + R : n;
  sh.n_prod = sh.sigagg ? sh.indiv_vbase : n;
  // the chunk groups' sum plan is staged with the inputs
  if (sh.sigagg && !sh.smsum) plan_gsum(req_off, plan.chunk_off, plan.chunk_reqs, pl.chunk_gsum);
  if (sh.use_units && !sh.smsum) plan_gsum_sets(pl.units.goff, pl.units.members, pl.unit_gsum);
  sh.use_total = sh.sigagg && !sh.sm && sh.merged && C > 1 && k.sig_total;
  sh.use_msm = sh.use_total && n <= MSM_MAX_SETS &&
               ((msm_on(k, env.in_flight) && !sh.merged_after_fail) || (flags & BLS_DEBUG_MSM));
  sh.msm_overlap = sh.use_msm && k.msm_overlap && !(flags & BLS_DEBUG_MSM_SERIAL);
  if (sh.use_total) {
    std::vector<uint32_t> goff(C + 1, (uint32_t)pl.chunk_gsum.gsets.size());
    goff[0] = 0;
    plan_gsum_sets(goff, pl.chunk_gsum.gsets, pl.total_gsum);
  }
  sh.gseg_cap = gseg_cap(n, R);
  sh.gtmp_cap = gtmp_cap(n, R);
  sh.ml_shared = sh.sigagg && k.ml_shared;
  if (sh.ml_shared) plan_ml_domains(req_off, plan, sh.use_units ? &pl.units : nullptr, n, pl.ml_dom);
  if (in->set_pk_offsets)
    for (uint32_t i = 0; i < n; ++i)
      if (in->set_pk_offsets[i + 1] - in->set_pk_offsets[i] >= BLS_AGG_WAVE_MIN) pl.agg_list.push_back(i);
  sh.fe_min = k.fe_simt_min;
  sh.fe_simt_possible = sh.fe_min > 0 && (C >= sh.fe_min || R >= sh.fe_min);
  sh.gt_min = group_test_min(k, flags);
  for (uint32_t ch = 0; ch < C && !sh.gt_possible; ++ch)
    sh.gt_possible = plan.chunk_off[ch + 1] - plan.chunk_off[ch] >= sh.gt_min;
  sh.grp_cap = sh.gt_possible ? grp_cap(R, C) : 0;
  sh.grp_mem_cap = sh.gt_possible ? grp_mem_cap(R) : 0;
  sh.gt_eq_mode = k.group_eq;
  sh.gsums_min = group_sums_min(k);
  sh.init_set_flag = (flags & BLS_DEBUG_FORCE_EXACT) ? 1u : 0u;
  sh.pack = (flags & BLS_DEBUG_PACK_MASK) >> 8;
  sh.mlf_pl = (flags & BLS_DEBUG_MLF_PL_MASK) >> 12;
  sh.pl_forced = (flags & BLS_DEBUG_MLF_PL_MASK) != 0;
  return sh;
}

// ---- verdicts -----------------------------------------------------------------------------

// Fill verdicts / stats from chunk results and the individual pass.
inline void assemble_verdicts(const bls_batch* in, const BatchPlan& p, const int32_t* chunk_ok,
                              const std::vector<uint32_t>& indiv_reqs, const int32_t* indiv_verdict,
                              int32_t* verdicts, bls_stats* stats) {
  uint32_t n_chunks = (uint32_t)p.chunk_off.size() - 1;
  uint32_t retries = 0, sigs_ok = 0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    if (chunk_ok[c] == 1) {
      for (uint32_t k = p.chunk_off[c]; k < p.chunk_off[c + 1]; ++k) {
        uint32_t r = p.chunk_reqs[k];
        verdicts[r] = 1;
        sigs_ok += in->req_set_offsets[r + 1] - in->req_set_offsets[r];
      }
    } else {
      ++retries;
    }
  }
  for (size_t t = 0; t < indiv_reqs.size(); ++t) verdicts[indiv_reqs[t]] = indiv_verdict[t];
  if (stats) {
    stats->batch_retries = retries;
    stats->batch_sigs_success = sigs_ok;
    stats->n_chunks = n_chunks;
    stats->n_individual = (uint32_t)indiv_reqs.size();
  }
}

}  // namespace bls
