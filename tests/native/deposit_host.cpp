// TEST INFRASTRUCTURE ONLY -- never linked into the product library.
//
// The per-deposit stage bodies of kernels/k_deposit.hip (bls/deposit.hpp: stage_deposit_root,
// stage_deposit_key, stage_deposit_pk) compiled for the host and run on records read from
// a file (argv[1]) or stdin, one per line, fields in hex:
//   root <pubkey 48> <withdrawal_credentials 32> <amount 8, little-endian> <domain 32>
//        -> "root <signing root 32>"
//   plan <n>
//        -> "plan <n> <rc of the shape check: 0 / -2> <chunks> <their sizes, comma separated>"
//           (bls/plan.hpp check_deposits, plan_deposits, plan_batch: the requests of a deposit call)
//   key <pubkey 48>
//        -> "key <code> <decoded point, 96 bytes uncompressed> <handed on: 0 infinity / 1 the point>"
// The decoded point is stage_deposit_key's (the infinity encoding when the bytes do not
// decode); "handed on" is what stage_deposit_pk leaves in b.pk for the later stages.  A
// stand-alone program (its own main), so it also runs under -fsanitize=address,undefined.
// Exit code 0, or 1 on a malformed record.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#define BLS_LAZY_POW 1
#include "bls/deposit.hpp"

unsigned long long bls_fpm_counter = 0;
unsigned long long bls_lz_norm_counter = 0;

using namespace bls;

static bool unhex(const std::string& s, size_t want, std::vector<uint8_t>& out) {
  if (s.size() != 2 * want) return false;
  out.resize(want);
  for (size_t i = 0; i < want; ++i) {
    unsigned v;
    if (sscanf(s.c_str() + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}

static void print_hex(const uint8_t* b, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", b[i]);
}

static std::vector<std::string> split(const char* line) {
  std::vector<std::string> out;
  std::string cur;
  for (const char* p = line;; ++p) {
    if (*p == ' ' || *p == '\n' || *p == '\r' || *p == 0) {
      if (!cur.empty()) out.push_back(cur);
      cur.clear();
      if (*p == 0) break;
    } else {
      cur.push_back(*p);
    }
  }
  return out;
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 1;
  }
  char line[1024];
  int lineno = 0;
  while (fgets(line, sizeof(line), f)) {
    ++lineno;
    const std::vector<std::string> w = split(line);
    if (w.empty()) continue;
    std::vector<uint8_t> pk, wc, amount, domain;
    if (w[0] == "root" && w.size() == 5 && unhex(w[1], 48, pk) && unhex(w[2], 32, wc) && unhex(w[3], 8, amount) &&
        unhex(w[4], 32, domain)) {
      uint8_t root[32];
      stage_deposit_root(pk.data(), wc.data(), amount.data(), domain.data(), root);
      printf("root ");
      print_hex(root, 32);
      printf("\n");
    } else if (w[0] == "plan" && w.size() == 2) {
      bls_deposit_batch in;
      memset(&in, 0, sizeof(in));
      in.n = (uint32_t)strtoul(w[1].c_str(), nullptr, 10);
      const uint8_t byte = 0;
      in.pubkeys48 = in.withdrawal_credentials = in.amounts = in.signatures = in.domain = &byte;  // never read here
      int32_t verdict = 0;
      if (check_deposits(&in, &verdict)) {
        printf("plan %u -2 0 -\n", in.n);
        continue;
      }
      DepositPlan dp;
      bls_batch all;
      plan_deposits(&in, dp, all);
      // request r owns set r and is batchable; the chunks are plan_batch's
      int rc = all.n_sets == in.n && all.n_reqs == in.n && !all.pubkeys && !all.set_pk_offsets && !all.messages ? 0 : -1;
      for (uint32_t r = 0; r <= in.n && rc == 0; ++r)
        if (all.req_set_offsets[r] != r || (r < in.n && all.req_batchable[r] != 1)) rc = -1;
      BatchPlan plan;
      plan_batch(&all, plan);
      if (!plan.nonbatch_reqs.empty() || plan.chunk_reqs.size() != in.n) rc = -1;
      const size_t chunks = in.n ? plan.chunk_off.size() - 1 : 0;
      printf("plan %u %d %zu ", in.n, rc, chunks);
      for (size_t c = 0; c < chunks; ++c) printf("%s%u", c ? "," : "", plan.chunk_off[c + 1] - plan.chunk_off[c]);
      printf("%s\n", chunks ? "" : "-");
    } else if (w[0] == "key" && w.size() == 2 && unhex(w[1], 48, pk)) {
      G1A a;
      const int32_t code = stage_deposit_key(pk.data(), a);
      uint8_t out96[96];
      g1_serialize96(a, out96);
      // the key stage over a one-deposit call
      G1J pk_out;
      int32_t st = -1;
      PipeBufs b;
      memset(&b, 0, sizeof(b));
      b.n_sets = 1;
      b.pk = &pk_out;
      b.pk_status = &st;
      DepositBufs d;
      memset(&d, 0, sizeof(d));
      d.pubkeys48 = pk.data();
      stage_deposit_pk(b, d, 0);
      if (st != code) {
        fprintf(stderr, "line %d: stage_deposit_pk status %d != stage_deposit_key code %d\n", lineno, st, code);
        return 1;
      }
      printf("key %d ", code);
      print_hex(out96, 96);
      printf(" %d\n", jac_is_inf(pk_out) ? 0 : 1);
    } else {
      fprintf(stderr, "line %d: malformed record\n", lineno);
      return 1;
    }
  }
  if (f != stdin) fclose(f);
  return 0;
}
