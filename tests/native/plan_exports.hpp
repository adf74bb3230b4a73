// TEST INFRASTRUCTURE ONLY -- never linked into the product library.
//
// C entry points over the host-side planners of a verify pass (bls/plan.hpp), for
// tests/test_plan_cpu.py through libhostsim.so (tests/native/hostsim.cpp) and for the
// stand-alone sanitizer program tests/native/plan_host.cpp.  Inputs are flat uint32 arrays;
// every call writes its result vectors one after another into `out` (cap words), each as
// its length followed by its items, and returns the words written, or -1 when they did
// not fit.
#pragma once

#include <vector>

#include "bls/group_decode.hpp"
#include "bls/plan.hpp"

namespace plan_exports {

struct Out {
  uint32_t* out;
  uint32_t cap, at = 0;
  void put(uint32_t x) {
    if (at < cap) out[at] = x;
    ++at;
  }
  void vec(const std::vector<uint32_t>& v) {
    put((uint32_t)v.size());
    for (uint32_t x : v) put(x);
  }
  int done() const { return at <= cap ? (int)at : -1; }
};

inline bls::BatchPlan batch_plan(const uint32_t* chunk_off, uint32_t n_chunks, const uint32_t* chunk_reqs,
                                 const uint32_t* nonbatch, uint32_t n_nonbatch) {
  bls::BatchPlan p;
  p.chunk_off.assign(chunk_off, chunk_off + n_chunks + 1);
  p.chunk_reqs.assign(chunk_reqs, chunk_reqs + chunk_off[n_chunks]);
  if (n_nonbatch) p.nonbatch_reqs.assign(nonbatch, nonbatch + n_nonbatch);
  return p;
}

inline int emit_gsum(const bls::GsumPlan& p, uint32_t* out, uint32_t cap) {
  Out o{out, cap};
  o.vec(p.gsets);
  o.vec(p.seg);
  o.vec(p.level_off);
  return o.done();
}

}  // namespace plan_exports

extern "C" {

// -> gsets, seg, level_off
int hs_plan_gsum_sets(const uint32_t* goff, uint32_t n_groups, const uint32_t* sets, uint32_t* out,
                             uint32_t cap) {
  bls::GsumPlan p;
  bls::plan_gsum_sets(std::vector<uint32_t>(goff, goff + n_groups + 1),
                      std::vector<uint32_t>(sets, sets + goff[n_groups]), p);
  return plan_exports::emit_gsum(p, out, cap);
}

int hs_plan_gsum(const uint32_t* req_off, const uint32_t* grp_off, uint32_t n_groups, const uint32_t* grp_reqs,
                        uint32_t* out, uint32_t cap) {
  bls::GsumPlan p;
  bls::plan_gsum(req_off, std::vector<uint32_t>(grp_off, grp_off + n_groups + 1),
                 std::vector<uint32_t>(grp_reqs, grp_reqs + grp_off[n_groups]), p);
  return plan_exports::emit_gsum(p, out, cap);
}

// which: 0 gseg_cap(n, R), 1 gtmp_cap(n, R), 2 grp_cap(R, C), 3 grp_mem_cap(R)
unsigned long long hs_plan_cap(int which, uint32_t n, uint32_t R, uint32_t C) {
  switch (which) {
    case 0: return bls::gseg_cap(n, R);
    case 1: return bls::gtmp_cap(n, R);
    case 2: return bls::grp_cap(R, C);
    default: return bls::grp_mem_cap(R);
  }
}

// plan_units (msg_rep: n entries) or, same_message != 0, units_same_message (msg_rep
// nullable) -> {used, n_units}, set_unit, unit_rep, unit_off, goff, members
int hs_plan_units(const uint32_t* req_off, const uint32_t* chunk_off, uint32_t n_chunks,
                         const uint32_t* chunk_reqs, const uint32_t* msg_rep, uint32_t n, int same_message,
                         uint32_t* out, uint32_t cap) {
  const bls::BatchPlan plan = plan_exports::batch_plan(chunk_off, n_chunks, chunk_reqs, nullptr, 0);
  std::vector<uint32_t> rep;
  if (msg_rep) rep.assign(msg_rep, msg_rep + n);
  bls::UnitPlan u;
  bool used = true;
  if (same_message) bls::units_same_message(plan, rep, n, u);
  else used = bls::plan_units(req_off, plan, rep, n, u);
  plan_exports::Out o{out, cap};
  o.vec({used ? 1u : 0u, u.n_units});
  o.vec(u.set_unit);
  o.vec(u.unit_rep);
  o.vec(u.unit_off);
  o.vec(u.goff);
  o.vec(u.members);
  return o.done();
}

// bounds: n_msgs + 1 -> chunk_off, chunk_reqs, nonbatch_reqs
int hs_plan_batch_msgs(const uint8_t* batchable, uint32_t n_reqs, const uint32_t* bounds, uint32_t n_msgs,
                              uint32_t* out, uint32_t cap) {
  bls_batch in;
  memset(&in, 0, sizeof(in));
  in.n_reqs = n_reqs;
  in.req_batchable = batchable;
  bls::BatchPlan p;
  bls::plan_batch_msgs(&in, std::vector<uint32_t>(bounds, bounds + n_msgs + 1), p);
  plan_exports::Out o{out, cap};
  o.vec(p.chunk_off);
  o.vec(p.chunk_reqs);
  o.vec(p.nonbatch_reqs);
  return o.done();
}

// unit_off: n_chunks + 1 entries, or nullptr for a pass without units -> dom
int hs_plan_ml_domains(const uint32_t* req_off, const uint32_t* chunk_off, uint32_t n_chunks,
                              const uint32_t* chunk_reqs, const uint32_t* nonbatch, uint32_t n_nonbatch,
                              const uint32_t* unit_off, uint32_t n, uint32_t* out, uint32_t cap) {
  const bls::BatchPlan plan = plan_exports::batch_plan(chunk_off, n_chunks, chunk_reqs, nonbatch, n_nonbatch);
  bls::UnitPlan u;
  if (unit_off) {
    u.unit_off.assign(unit_off, unit_off + n_chunks + 1);
    u.n_units = unit_off[n_chunks];
  }
  std::vector<uint32_t> dom;
  bls::plan_ml_domains(req_off, plan, unit_off ? &u : nullptr, n, dom);
  plan_exports::Out o{out, cap};
  o.vec(dom);
  return o.done();
}

// -> reqs, the group-tested chunks as (beg, end, chunk) triples, {n_direct}
int hs_plan_indiv(const uint32_t* chunk_off, uint32_t n_chunks, const uint32_t* chunk_reqs,
                         const uint32_t* nonbatch, uint32_t n_nonbatch, const int32_t* chunk_ok, uint32_t gt_min,
                         uint32_t* out, uint32_t cap) {
  const bls::BatchPlan plan = plan_exports::batch_plan(chunk_off, n_chunks, chunk_reqs, nonbatch, n_nonbatch);
  bls::IndivPlan p;
  bls::plan_indiv(plan, chunk_ok, gt_min, p);
  std::vector<uint32_t> gt;
  for (const bls::GtChunk& c : p.gt_chunks) gt.insert(gt.end(), {c.beg, c.end, c.ch});
  plan_exports::Out o{out, cap};
  o.vec(p.reqs);
  o.vec(gt);
  o.vec({p.n_direct});
  return o.done();
}

// runs == 0: plan_own_sets(all, set_unit nullable) -> the sets; else plan_own_runs -> (first, count) pairs
int hs_plan_own_sets(const uint32_t* req_off, const uint32_t* reqs, uint32_t n_reqs, uint32_t first_t, int all,
                            const uint32_t* set_unit, int runs, uint32_t* out, uint32_t cap) {
  const std::vector<uint32_t> r(reqs, reqs + n_reqs);
  std::vector<uint32_t> own;
  if (runs) bls::plan_own_runs(req_off, r, first_t, own);
  else bls::plan_own_sets(req_off, r, first_t, all != 0, set_unit, own);
  plan_exports::Out o{out, cap};
  o.vec(own);
  return o.done();
}

// -> groups, {n_fold1, any_fold}
int hs_plan_fold_groups(const uint32_t* req_off, const uint32_t* reqs, uint32_t n_reqs, uint32_t* out,
                               uint32_t cap) {
  bls::FoldPlan f;
  bls::plan_fold_groups(req_off, std::vector<uint32_t>(reqs, reqs + n_reqs), f);
  plan_exports::Out o{out, cap};
  o.vec(f.groups);
  o.vec({f.n_fold1, f.any_fold ? 1u : 0u});
  return o.done();
}

// gt: n_gt (beg, end, chunk) triples; verdict: the indiv verdicts -> off, members, ref,
// per chunk kept (first, nbits, whole, has_err, n_ok), the chunks' ok lists concatenated
int hs_plan_group_tests_a(const uint32_t* gt, uint32_t n_gt, const int32_t* verdict, int eq, int chunk_fe,
                                 uint32_t* out, uint32_t cap) {
  std::vector<bls::GtChunk> chunks;
  for (uint32_t k = 0; k < n_gt; ++k) chunks.push_back({gt[3 * k], gt[3 * k + 1], gt[3 * k + 2]});
  bls::GroupTestsA a;
  bls::plan_group_tests_a(chunks, verdict, eq != 0, chunk_fe != 0, a);
  std::vector<uint32_t> cs, ok;
  for (const bls::GroupTestChunk& c : a.cs) {
    cs.insert(cs.end(), {c.first, c.nbits, c.whole ? 1u : 0u, c.has_err ? 1u : 0u, (uint32_t)c.ok.size()});
    ok.insert(ok.end(), c.ok.begin(), c.ok.end());
  }
  plan_exports::Out o{out, cap};
  o.vec(a.off);
  o.vec(a.members);
  o.vec(a.ref);
  o.vec(cs);
  o.vec(ok);
  return o.done();
}

int hs_check_batch(const bls_batch* in, const char* what, char* err, uint32_t err_len) {
  return bls::check_batch(in, what, err, err_len);
}

}  // extern "C"
