// TEST INFRASTRUCTURE ONLY -- never linked into the product library.
//
// C entry points over the host-side planners of a verify pass (bls/plan.hpp) and the knobs
// they are steered by (bls/knobs.hpp), for tests/test_plan_cpu.py and
// tests/test_knobs_cpu.py through libhostsim.so (tests/native/hostsim.cpp) and for the
// stand-alone sanitizer program tests/native/plan_host.cpp.  Inputs are flat uint32 arrays;
// every call writes its result vectors one after another into `out` (cap words), each as
// its length followed by its items, and returns the words written, or -1 when they did
// not fit.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "bls/group_decode.hpp"
#include "bls/knobs.hpp"
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

// bls::knobs_parse over an environment given as text: NAME=VALUE lines (an empty VALUE is
// a variable set to the empty string; a name without a line is unset)
inline std::vector<std::pair<std::string, std::string>>& knob_env() {
  static std::vector<std::pair<std::string, std::string>> env;
  return env;
}
inline const char* knob_get(const char* name) {
  for (const auto& kv : knob_env())
    if (kv.first == name) return kv.second.c_str();
  return nullptr;
}
inline bls::Knobs knobs_of(const char* text) {
  knob_env().clear();
  for (const char* p = text ? text : ""; *p;) {
    const char* end = strchr(p, '\n');
    const std::string line(p, end ? (size_t)(end - p) : strlen(p));
    const size_t eq = line.find('=');
    if (eq != std::string::npos) knob_env().emplace_back(line.substr(0, eq), line.substr(eq + 1));
    p += line.size() + (end ? 1 : 0);
  }
  return bls::knobs_parse(knob_get);
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

// ---- bls/knobs.hpp and plan_pass: the environment is `text`, NAME=VALUE lines ---------------

// "NAME\tdescription\n" per knob, in table order; returns the bytes written or -1
int hs_knob_table(char* out, uint32_t cap) {
  size_t n_rows;
  const bls::KnobRow* rows = bls::knob_rows(&n_rows);
  std::string s;
  for (size_t k = 0; k < n_rows; ++k) s += std::string(rows[k].name) + "\t" + rows[k].doc + "\n";
  if (s.size() + 1 > cap) return -1;
  memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

// -> every field in table order, each as the (low, high) words of its value as an int64
int hs_knobs_parse(const char* text, uint32_t* out, uint32_t cap) {
  const bls::Knobs k = plan_exports::knobs_of(text);
  std::vector<uint32_t> v;
#define X(name, type, field, kind, unset, doc) \
  v.push_back((uint32_t)(uint64_t)(int64_t)k.field), v.push_back((uint32_t)((uint64_t)(int64_t)k.field >> 32));
  BLS_KNOB_TABLE(X)
#undef X
  plan_exports::Out o{out, cap};
  o.vec(v);
  return o.done();
}

// which: 0 use_sigagg(k, flags, n, in_flight), 1 msm_on(k, in_flight), 2 group_test_min(k, flags),
// 3 group_sums_min(k), 4 wait_blocks(k, n), 5 mlf_per_lane(k, in_flight), 6 mlf_per_lane_alone(k, n),
// 7 pack_for(k, n, in_flight)
unsigned long long hs_knob_decide(const char* text, int which, uint32_t flags, uint32_t n,
                                  unsigned long long in_flight) {
  const bls::Knobs k = plan_exports::knobs_of(text);
  switch (which) {
    case 0: return bls::use_sigagg(k, flags, n, in_flight);
    case 1: return bls::msm_on(k, in_flight);
    case 2: return bls::group_test_min(k, flags);
    case 3: return bls::group_sums_min(k);
    case 4: return bls::wait_blocks(k, n);
    case 5: return bls::mlf_per_lane(k, in_flight);
    case 6: return bls::mlf_per_lane_alone(k, n);
    default: return bls::pack_for(k, n, in_flight);
  }
}

// plan_pass as VerifyPass calls it.  The batch: R requests over the sets req_off names,
// set i one table key signing root roots[i] (its 32-byte message holds that number).
// ask: 0 a verify call (bounds: verify_many's n_msgs + 1 first requests, or nullptr), 1 a
// partial call, 2 a deposit call (neither keys nor messages), 3 a same-message call of the
// jobs job_off[0 .. n_jobs] over one-set requests (batchable is then the plan's).
// -> the PassShape fields (the order below; gsums_min capped at 0xFFFFFFFF), the plans'
// sizes {chunk_gsum.gsets, unit_gsum.gsets, total_gsum.gsets, total_gsum levels, ml_dom,
// agg_list, msg_uniq}, chunk_off
int hs_plan_pass(const char* text, const uint32_t* req_off, uint32_t R, const uint8_t* batchable,
                 const uint32_t* roots, int ask, const uint32_t* aux, uint32_t n_aux, uint32_t flags,
                 int last_merged_failed, unsigned long long in_flight, uint32_t* out, uint32_t cap) {
  const uint32_t n = req_off[R];
  std::vector<uint8_t> msgs(32ull * n + 1, 0), flag(batchable, batchable + R);
  for (uint32_t i = 0; i < n; ++i) memcpy(&msgs[32ull * i], &roots[i], 4);
  std::vector<uint32_t> pk_off(n + 1), pk_idx(n + 1, 0);
  for (uint32_t i = 0; i <= n; ++i) pk_off[i] = i;
  bls_batch in;
  memset(&in, 0, sizeof(in));
  in.n_sets = n;
  in.n_reqs = R;
  in.req_set_offsets = req_off;
  bls::SameMsgPlan sm;
  std::vector<uint32_t> bounds;
  bls::PassAsk a{ask == 1, nullptr, ask == 2, nullptr};
  if (ask == 3) {
    bls_same_msg_batch jobs;
    memset(&jobs, 0, sizeof(jobs));
    jobs.n_jobs = n_aux;
    jobs.n_sets = n;
    jobs.job_set_offsets = aux;
    bls::plan_same_message(&jobs, sm);
    flag.assign(R, 1);
    for (uint32_t r : sm.plan.nonbatch_reqs) flag[r] = 0;
    a.sm = &sm;
  } else if (aux) {
    bounds.assign(aux, aux + n_aux + 1);
    a.req_bounds = &bounds;
  }
  in.req_batchable = flag.data();
  if (ask != 2) {
    in.set_pk_offsets = pk_off.data();
    in.pk_indices = pk_idx.data();
    in.messages = msgs.data();
  }
  const bls::Knobs k = plan_exports::knobs_of(text);
  bls::PassPlans pl;
  const bls::PassShape sh =
      bls::plan_pass(&in, a, bls::PassEnv{flags, last_merged_failed != 0, in_flight}, k, pl);
  auto cap32 = [](size_t x) { return x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)x; };
  plan_exports::Out o{out, cap};
  o.vec({sh.n, sh.R, sh.n_chunks, sh.n_uniq, sh.n_pk_idx, sh.partial, sh.sm, sh.dedup, sh.dep, sh.merged_eligible,
         sh.merged_skipped, sh.merged, sh.sigagg, sh.use_units, sh.smsum, sh.use_total, sh.use_msm, sh.msm_overlap,
         sh.ml_shared, sh.n_units, sh.unit_base, sh.indiv_vbase, sh.n_total, sh.n_prod, sh.gt_min, sh.gt_possible,
         (uint32_t)sh.gt_eq_mode, cap32(sh.gsums_min), sh.fe_min, sh.fe_simt_possible, sh.init_set_flag, sh.pack,
         sh.mlf_pl, sh.pl_forced, sh.merged_after_fail, cap32(sh.gseg_cap), cap32(sh.gtmp_cap), cap32(sh.grp_cap),
         cap32(sh.grp_mem_cap)});
  o.vec({(uint32_t)pl.chunk_gsum.gsets.size(), (uint32_t)pl.unit_gsum.gsets.size(),
         (uint32_t)pl.total_gsum.gsets.size(), (uint32_t)pl.total_gsum.level_off.size(), (uint32_t)pl.ml_dom.size(),
         (uint32_t)pl.agg_list.size(), (uint32_t)pl.msg_uniq.size()});
  o.vec(pl.plan->chunk_off);
  return o.done();
}

}  // extern "C"
