// TEST INFRASTRUCTURE ONLY -- never linked into the product library.
//
// The host-side planners of a verify pass (bls/plan.hpp) run through their C entry points
// (plan_exports.hpp, the ones tests/test_plan_cpu.py calls) over the edge shapes of that
// test, as a stand-alone program (its own main) so that it also runs under
// -fsanitize=address,undefined: an index past a plan's vectors or the caller's arrays is a
// report there.  The program re-checks the invariants the device relies on (segments
// inside their group and level, every set in exactly one unit, runs inside the requests);
// the value checks against a Python restatement are tests/test_plan_cpu.py's.  It also
// parses every knob (bls/knobs.hpp) and runs plan_pass, the decision table of a whole
// pass, over the shapes of tests/test_knobs_cpu.py (which checks their values).
//
//   plan_host            prints "ok <checks>" and exits 0, or the first mismatch and 1
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "plan_exports.hpp"

using namespace bls;
typedef std::vector<uint32_t> U32s;

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

// the vectors of one call's output
static std::vector<U32s> parse(const U32s& out, int words) {
  std::vector<U32s> v;
  for (size_t at = 0; at < (size_t)words;) {
    const uint32_t len = out[at++];
    v.emplace_back(out.begin() + at, out.begin() + at + len);
    at += len;
  }
  return v;
}

static U32s offsets(const U32s& sizes) {
  U32s off(1, 0);
  for (uint32_t s : sizes) off.push_back(off.back() + s);
  return off;
}

// replay the levels over integer "points": every group's sum must come out, in order
static int gsum_case(const U32s& sizes) {
  const U32s goff = offsets(sizes);
  const uint32_t n = goff.back(), G = (uint32_t)sizes.size();
  U32s sets(n);
  for (uint32_t i = 0; i < n; ++i) sets[i] = n - 1 - i;  // any order: the plan only indexes them
  U32s out(16 * n + 64 * G + 64);
  const int w = hs_plan_gsum_sets(goff.data(), G, sets.data(), out.data(), (uint32_t)out.size());
  CHECK(w > 0, "plan_gsum_sets output does not fit");
  const std::vector<U32s> v = parse(out, w);
  const U32s &gsets = v[0], &seg = v[1], &lvl = v[2];
  CHECK(gsets == sets && lvl.size() >= 2 && lvl[0] == 0 && 2 * lvl.back() == seg.size(), "plan layout");
  CHECK(seg.size() <= hs_plan_cap(0, n, G, 0) && lvl[1] <= hs_plan_cap(1, n, G, 0), "plan exceeds the caps");
  std::vector<uint64_t> cur;
  for (uint32_t i : gsets) cur.push_back(i + 1);
  for (size_t L = 0; L + 1 < lvl.size(); ++L) {
    std::vector<uint64_t> next;
    for (uint32_t k = lvl[L]; k < lvl[L + 1]; ++k) {
      const uint32_t beg = seg[2 * k], end = seg[2 * k + 1];
      CHECK(beg <= end && end <= cur.size() && end - beg <= GSUM_FAN, "level %zu segment %u = [%u, %u)", L, k, beg, end);
      uint64_t sum = 0;
      for (uint32_t i = beg; i < end; ++i) sum += cur[i];
      next.push_back(sum);
    }
    cur.swap(next);
  }
  CHECK(cur.size() == G, "%zu sums for %u groups", cur.size(), G);
  for (uint32_t g = 0; g < G; ++g) {
    uint64_t want = 0;
    for (uint32_t k = goff[g]; k < goff[g + 1]; ++k) want += sets[k] + 1;
    CHECK(cur[g] == want, "group %u sum", g);
  }
  return 0;
}

// chunks of one-set requests with the given roots: units partition each chunk's sets
static int units_case(const U32s& chunk_sizes, const U32s& root_of_set, bool expect_used) {
  const U32s chunk_off = offsets(chunk_sizes);
  const uint32_t n = chunk_off.back(), C = (uint32_t)chunk_sizes.size();
  U32s req_off(n + 1), chunk_reqs(n), rep(n);
  for (uint32_t i = 0; i <= n; ++i) req_off[i] = i;
  for (uint32_t i = 0; i < n; ++i) {
    chunk_reqs[i] = i;
    rep[i] = i;
    for (uint32_t j = 0; j < i; ++j)
      if (root_of_set[j] == root_of_set[i]) {
        rep[i] = j;
        break;
      }
  }
  for (int sm = 0; sm < 2; ++sm) {
    U32s out(8 * n + 64);
    const int w = hs_plan_units(req_off.data(), chunk_off.data(), C, chunk_reqs.data(), rep.data(), n, sm, out.data(),
                                (uint32_t)out.size());
    CHECK(w > 0, "plan_units output does not fit");
    const std::vector<U32s> v = parse(out, w);
    const bool used = v[0][0] != 0;
    CHECK(sm || used == expect_used, "units used = %d", (int)used);
    if (!used) continue;
    const U32s &set_unit = v[1], &unit_rep = v[2], &unit_off = v[3], &goff = v[4], &mem = v[5];
    const uint32_t U = v[0][1];
    CHECK(unit_off.size() == C + 1 && unit_off[C] == U && goff.size() == U + 1 && mem.size() == n, "unit layout");
    U32s seen(n, 0);
    for (uint32_t c = 0; c < C; ++c)
      for (uint32_t u = unit_off[c]; u < unit_off[c + 1]; ++u)
        for (uint32_t k = goff[u]; k < goff[u + 1]; ++k) {
          const uint32_t i = mem[k];
          CHECK(i >= chunk_off[c] && i < chunk_off[c + 1] && set_unit[i] == u && !seen[i]++, "set %u in unit %u", i, u);
          // (a same-message unit is its whole chunk, whatever the roots say)
          CHECK(sm || root_of_set[unit_rep[u]] == root_of_set[i], "unit %u: representative of another root", u);
        }
    // the domains of the same pass: every item's chunk
    U32s dom(n + C + U + 8);
    const int wd = hs_plan_ml_domains(req_off.data(), chunk_off.data(), C, chunk_reqs.data(), nullptr, 0,
                                      unit_off.data(), n, dom.data(), (uint32_t)dom.size());
    CHECK(wd == (int)(n + C + U + 1), "plan_ml_domains: %d words", wd);
  }
  return 0;
}

// the individually verified list of a pass and everything planned from it
static int indiv_case(const U32s& req_sizes, const std::vector<uint8_t>& batchable, const U32s& bounds,
                      uint32_t gt_min) {
  const U32s req_off = offsets(req_sizes);
  const uint32_t R = (uint32_t)req_sizes.size(), n = req_off.back();
  U32s out(4 * R + 64);
  int w = hs_plan_batch_msgs(batchable.data(), R, bounds.data(), (uint32_t)bounds.size() - 1, out.data(),
                             (uint32_t)out.size());
  CHECK(w > 0, "plan_batch_msgs output does not fit");
  const std::vector<U32s> bp = parse(out, w);
  const U32s &chunk_off = bp[0], &chunk_reqs = bp[1], &nonbatch = bp[2];
  const uint32_t C = (uint32_t)chunk_off.size() - 1;
  CHECK(chunk_reqs.size() + nonbatch.size() == R && chunk_off[C] == chunk_reqs.size(), "batch plan layout");
  std::vector<int32_t> chunk_ok(C + 1, 1);
  for (uint32_t c = 0; c < C; c += 2) chunk_ok[c] = 0;  // every other chunk failed
  w = hs_plan_indiv(chunk_off.data(), C, chunk_reqs.data(), nonbatch.data(), (uint32_t)nonbatch.size(),
                    chunk_ok.data(), gt_min, out.data(), (uint32_t)out.size());
  CHECK(w > 0, "plan_indiv output does not fit");
  const std::vector<U32s> ip = parse(out, w);
  const U32s &reqs = ip[0], &gt = ip[1];
  const uint32_t n_direct = ip[2][0];
  CHECK(n_direct <= reqs.size() && reqs.size() <= R, "indiv list");
  for (size_t k = 0; k < gt.size(); k += 3)
    CHECK(gt[k] >= n_direct && gt[k] < gt[k + 1] && gt[k + 1] <= reqs.size() && gt[k + 2] < C, "group-tested chunk");

  U32s big(2 * n + 4 * R + 64);
  for (int variant = 0; variant < 3; ++variant) {
    w = hs_plan_own_sets(req_off.data(), reqs.data(), (uint32_t)reqs.size(), (uint32_t)nonbatch.size(), variant == 0,
                         nullptr, variant == 2, big.data(), (uint32_t)big.size());
    CHECK(w > 0, "plan_own_sets output does not fit");
    const U32s own = parse(big, w)[0];
    if (variant == 2)
      for (size_t k = 0; k < own.size(); k += 2) CHECK(own[k + 1] > 0 && own[k] + own[k + 1] <= n, "run past the sets");
    else
      for (uint32_t i : own) CHECK(i < n, "own set %u", i);
  }
  w = hs_plan_fold_groups(req_off.data(), reqs.data(), (uint32_t)reqs.size(), big.data(), (uint32_t)big.size());
  CHECK(w > 0, "plan_fold_groups output does not fit");
  const std::vector<U32s> fp = parse(big, w);
  // the workspace bls_gpu.hip carves for them
  CHECK(fp[0].size() <= 2ull * (n / BLS_FOLD1 + R + 1) + 2ull * (n / BLS_FOLD + R + 1), "fold groups exceed the carve");
  for (size_t k = 0; k < fp[0].size(); k += 2) {
    const uint32_t span = fp[0][k + 1] - fp[0][k];
    CHECK(fp[0][k] < fp[0][k + 1] && fp[0][k + 1] <= n && span <= (k / 2 < fp[1][0] ? BLS_FOLD1 : BLS_FOLD), "fold group");
  }

  // group tests over the group-tested chunks, one request erroneous, both modes
  std::vector<int32_t> verdict(reqs.size() + 1, 2);
  if (!gt.empty()) verdict[gt[0]] = -3;
  for (int mode = 0; mode < 4; ++mode) {
    U32s go(16 * R + 64 * C + 64);
    w = hs_plan_group_tests_a(gt.data(), (uint32_t)gt.size() / 3, verdict.data(), mode & 1, mode >> 1, go.data(),
                              (uint32_t)go.size());
    CHECK(w > 0, "plan_group_tests_a output does not fit");
    const std::vector<U32s> ga = parse(go, w);
    const U32s &off = ga[0], &mem = ga[1], &ref = ga[2];
    CHECK(off.size() == ref.size() + 1 && off.back() == mem.size(), "group-test layout");
    CHECK(mem.size() <= hs_plan_cap(3, n, R, C) && ref.size() <= hs_plan_cap(2, n, R, C), "group tests exceed the caps");
    for (uint32_t t : mem) CHECK(t >= n_direct && t < reqs.size() && verdict[t] == 2, "group-test member %u", t);
    for (size_t t = 0; (mode & 1) && t < ref.size(); ++t)  // (without eq the refs are not staged)
      CHECK(ref[t] == REF_NONE || ((ref[t] & REF_CHUNK) ? (ref[t] & ~REF_CHUNK) < C : ref[t] < t), "ref of test %zu", t);
  }
  return 0;
}

static int check_batch_cases() {
  const uint32_t off[] = {0, 1, 2}, back[] = {0, 2, 1}, pk_off[] = {0, 1, 2}, idx[] = {0, 0};
  uint8_t bytes[192] = {0};
  char err[128];
  bls_batch in;
  memset(&in, 0, sizeof(in));
  in.n_sets = 2;
  in.n_reqs = 2;
  CHECK(hs_check_batch(&in, "b", err, sizeof(err)) == -2 && strstr(err, "req_set_offsets missing"), "%s", err);
  in.req_set_offsets = off;
  in.set_pk_offsets = pk_off;
  in.pk_indices = idx;
  in.messages = in.signatures = bytes;
  CHECK(hs_check_batch(&in, "b", err, sizeof(err)) == 0, "a good batch: %s", err);
  in.req_set_offsets = back;
  CHECK(hs_check_batch(&in, "b", err, sizeof(err)) == -2, "offsets that go back");
  return 0;
}

// every knob parsed from an environment that sets it (to `value`) and from one that does
// not; the table's names are distinct
static int knobs_cases() {
  char table[1 << 14];
  CHECK(hs_knob_table(table, sizeof(table)) > 0, "knob table does not fit");
  std::vector<std::string> names;
  for (const char* p = table; *p; p = strchr(p, '\n') + 1) names.emplace_back(p, strchr(p, '\t') - p);
  for (size_t a = 0; a < names.size(); ++a)
    for (size_t b = 0; b < a; ++b) CHECK(names[a] != names[b], "knob %s twice", names[a].c_str());
  U32s out(4 * names.size() + 8);
  for (const char* value : {"", "0", "1", "3", "-1", "poll", "18446744073709551615"}) {
    std::string all;
    for (const std::string& nm : names) {
      const std::string one = nm + "=" + value + "\n";
      CHECK(hs_knobs_parse(one.c_str(), out.data(), (uint32_t)out.size()) == (int)(1 + 2 * names.size()), "%s", nm.c_str());
      all += one;
    }
    CHECK(hs_knobs_parse(all.c_str(), out.data(), (uint32_t)out.size()) > 0, "all knobs = %s", value);
    for (int which = 0; which < 8; ++which)
      for (unsigned long long in_flight : {0ull, 60001ull, ~0ull}) (void)hs_knob_decide(all.c_str(), which, 0, 2049, in_flight);
  }
  CHECK(hs_knobs_parse("", out.data(), (uint32_t)out.size()) > 0 && hs_knobs_parse(nullptr, out.data(), (uint32_t)out.size()) > 0,
        "no environment");
  return 0;
}

// plan_pass over one batch: the layout the carve and the kernels rely on
static int pass_case(const char* env, const U32s& req_sizes, const std::vector<uint8_t>& batchable, const U32s& roots,
                     int ask, const U32s& aux, uint32_t flags, int failed, unsigned long long in_flight) {
  const U32s req_off = offsets(req_sizes);
  const uint32_t R = (uint32_t)req_sizes.size(), n = req_off.back();
  U32s out(256 + R);
  const int w = hs_plan_pass(env, req_off.data(), R, batchable.data(), roots.data(), ask, aux.empty() ? nullptr : aux.data(),
                             aux.empty() ? 0u : (uint32_t)aux.size() - 1, flags, failed, in_flight, out.data(),
                             (uint32_t)out.size());
  CHECK(w > 0, "plan_pass output does not fit");
  const std::vector<U32s> v = parse(out, w);
  const U32s &sh = v[0], &sizes = v[1], &chunk_off = v[2];
  const uint32_t C = (uint32_t)chunk_off.size() - 1;
  const uint32_t sigagg = sh[12], n_units = sh[19], unit_base = sh[20], indiv_vbase = sh[21], n_total = sh[22];
  CHECK(sh[0] == n && sh[1] == R && sh[2] == C, "n, R, C");
  CHECK(unit_base == n + C && indiv_vbase == unit_base + n_units, "unit_base %u indiv_vbase %u", unit_base, indiv_vbase);
  CHECK(n_total == (sigagg ? indiv_vbase + R : n) && sh[23] == (sigagg ? indiv_vbase : n), "n_total %u", n_total);
  CHECK(sh[11] == (sh[9] && !sh[10]), "merged = eligible and not skipped");
  CHECK(sh[17] <= sh[16] && sh[16] <= sh[15] && sh[15] <= sh[11] && sh[15] <= sigagg, "msm_overlap <= use_msm <= use_total");
  CHECK(sizes[0] <= n && sizes[1] <= n && sizes[2] <= n, "a sum plan over more than the sets");
  CHECK(sizes[4] == (sh[18] ? unit_base + n_units : 0u), "ml_dom of %u items", sizes[4]);
  return 0;
}

static int pass_cases() {
  U32s ones(64, 1), distinct(64), shared(64), none;
  for (uint32_t i = 0; i < 64; ++i) distinct[i] = i, shared[i] = i / 8;
  const std::vector<uint8_t> all(70, 1);
  std::vector<uint8_t> some(all);
  some[30] = 0;
  const uint32_t on = BLS_DEBUG_SIGAGG_ON, off = BLS_DEBUG_SIGAGG_OFF;
  for (uint32_t flags : {on, off, on | BLS_DEBUG_MSM, on | BLS_DEBUG_MSM | BLS_DEBUG_MSM_SERIAL, on | BLS_DEBUG_NO_UNITS,
                         on | BLS_DEBUG_MERGED_EVERY_PASS, on | BLS_DEBUG_NO_MSG_DEDUP, 0u})
    for (int failed = 0; failed < 2; ++failed)
      for (unsigned long long in_flight : {0ull, 60001ull}) {
        for (int ask = 0; ask < 3; ++ask)
          if (pass_case("", ones, all, ask ? distinct : shared, ask, none, flags, failed, in_flight)) return 1;
        if (pass_case("BLS_MERGED_AFTER_FAIL=1\n", ones, some, shared, 0, none, flags, failed, in_flight)) return 1;
        if (pass_case("", ones, all, distinct, 0, {0, 40, 64}, flags, failed, in_flight)) return 1;
        if (pass_case("", ones, all, shared, 3, {0, 20, 64}, flags, failed, in_flight)) return 1;
        if (pass_case("", ones, all, shared, 3, {0, 20, 21, 64}, flags, failed, in_flight)) return 1;
      }
  // 16 requests (one chunk), 3 and 4 (group tests), requests of 0 .. 5 sets, no set at all
  for (uint32_t R : {16u, 3u, 4u}) if (pass_case("", U32s(R, 1), all, distinct, 0, none, on, 0, 0)) return 1;
  U32s mixed(70), roots;
  for (uint32_t r = 0; r < 70; ++r) mixed[r] = (7 * r) % 6;
  for (uint32_t i = 0; i < offsets(mixed).back(); ++i) roots.push_back(i / 6);
  for (uint32_t flags : {on, off})
    if (pass_case("", mixed, all, roots, 0, none, flags, 0, 1000000) || pass_case("", mixed, some, roots, 1, none, flags, 1, 0)) return 1;
  if (pass_case("", {0, 0}, all, none, 0, none, on, 0, 60001)) return 1;
  return 0;
}

int main() {
  if (knobs_cases() || pass_cases()) return 1;
  const U32s sizes = {0, 1, 4, 5, 16, 17, 65};
  if (gsum_case(sizes) || gsum_case({65, 17, 16, 5, 4, 1, 0}) || gsum_case({0, 65, 0}) || gsum_case({0})) return 1;
  // two chunks of 16 one-set requests, roots shared 8-way inside a chunk and across both
  U32s roots(32);
  for (uint32_t i = 0; i < 32; ++i) roots[i] = (i % 16) / 8;
  if (units_case({16, 16}, roots, true)) return 1;
  for (uint32_t i = 0; i < 32; ++i) roots[i] = i < 20 ? i : 0;  // too many units: refused
  if (units_case({16, 16}, roots, false)) return 1;
  // messages of 0, 15, 16, 33 and 40 batchable requests, non-batchable ones interleaved
  U32s req_sizes, bounds(1, 0);
  std::vector<uint8_t> batchable;
  const uint32_t per_msg[] = {0, 15, 16, 33, 40};
  const uint32_t set_sizes[] = {1, 4, 5, 16, 17, 33, 0, 2};
  for (uint32_t m = 0; m < 5; ++m) {
    for (uint32_t k = 0; k < per_msg[m]; ++k) {
      batchable.push_back(1);
      req_sizes.push_back(set_sizes[(k + m) % 8]);
      if (k % 7 == 3) {
        batchable.push_back(0);
        req_sizes.push_back(set_sizes[k % 8]);
      }
    }
    batchable.push_back(0);
    req_sizes.push_back(3);
    bounds.push_back((uint32_t)batchable.size());
  }
  if (indiv_case(req_sizes, batchable, bounds, 4) || indiv_case(req_sizes, batchable, bounds, 17)) return 1;
  if (check_batch_cases()) return 1;
  printf("ok %d\n", g_checks);
  return 0;
}
