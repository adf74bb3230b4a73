// Pubkey stage: deserialize raw 96-byte keys or sum device-table keys (aggregate sets given
// as index lists, as a registered committee and its participation bits, or as a span of
// committees under one field), plus the
// pubkey-table loader and the per-request status pass (small kernels).
#include "../launchers.hpp"

using namespace bls;

// First kernel of a verify call: also resets the call's device-side words, so the
// call needs no memset blits (which queue behind every context's copies and wait for
// CU slots under load): set_flag (the exact-path marks), flag_count, and the other
// slot of the two-slot first_bad_pk (the next call's; this call's slot was reset by
// the previous call, or at context creation).
__global__ __launch_bounds__(BLS_BLOCK) void k_pk(PipeBufs b) {
  const uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i < b.n_sets) b.set_flag[i] = b.init_set_flag;
  if (i == 0) {
    *b.flag_count = 0u;
    if (b.first_bad_pk_next) *b.first_bad_pk_next = 0xFFFFFFFFu;
  }
  stage_pk(b, i);
}

// getAggregatedPubkey (chain/bls/utils.ts:5-16) as a reduction, one wavefront per
// aggregate set of >= agg_min keys (b.agg_sets): lane l sums keys l, l + 64, ... of the
// set with mixed additions (table points are affine), then six levels of a tree over the
// lanes' partial sums in LDS.  An aggregate of k keys costs ceil(k / 64) + 6 additions
// of latency instead of k - 1 (cfg3's 512-key aggregates: 14 instead of 511).  The sum
// is a group element, so the order of additions changes nothing downstream (every
// consumer works on the point: the serialized aggregate is its canonical affine form).
// Table gathers stay array-of-structures: a key is one random 100-byte read.
__global__ __launch_bounds__(BLS_BLOCK) void k_pk_agg(PipeBufs b) {
  __shared__ G1J part[BLS_BLOCK];
  const uint32_t lane = threadIdx.x;
  const uint32_t i = b.agg_sets[blockIdx.x];
  const uint32_t beg = b.set_pk_off[i], end = b.set_pk_off[i + 1];
  G1J acc = jac_infinity<Fp>();
  bool bad = false;
  for (uint32_t k = beg + lane; k < end; k += BLS_BLOCK) {
    const uint32_t idx = b.pk_idx[k];
    if (idx >= b.pk_table_n) bad = true;
    else acc = jac_add_aff(acc, b.pk_table[idx]);
  }
  part[lane] = acc;
  __syncthreads();
  for (uint32_t s = BLS_BLOCK / 2; s >= 1; s >>= 1) {
    if (lane < s) part[lane] = jac_add(part[lane], part[lane + s]);
    __syncthreads();
  }
  const bool any_bad = __any(bad);
  if (lane == 0) {
    const G1J sum = part[0];
    b.pk[i] = sum;
    b.pk_status[i] = any_bad ? BLS_BAD_ENCODING : BLS_OK;
    if (b.pk_inf) b.pk_inf[i] = (!any_bad && jac_is_inf(sum)) ? 1 : 0;
  }
}

hipError_t launch_k_pk_agg(const PipeBufs& b, hipStream_t s) {
  if (b.n_agg == 0) return hipSuccess;
  k_pk_agg<<<b.n_agg, BLS_BLOCK, 0, s>>>(b);
  return hipGetLastError();
}

// The selected members of one committee summed by a wavefront (bls/committee.hpp): position
// j of mem[0, n) is summed when bits is null (every member: a committee's total) or
// committee_selects(bits, j, comp).  The selected positions are compacted round by round --
// a ballot over 64 positions, each selected lane's rank by the prefix count -- into a
// 128-entry ring in LDS that the lanes drain 64 at a time, so a lane does at most
// ceil(selected / 64) mixed additions wherever the bits fall (a lane per position would
// hand one lane every selected member of a field whose set bits lie 64 apart).  Then
// k_pk_agg's six-level tree; part[0] holds the sum.  Every loop bound is uniform over the wavefront.  bad: a member at or past
// the table (registration rules it out; the read is not made).
__device__ __forceinline__ void committee_wave_sum(G1J* part, uint32_t* ring, const uint32_t* mem, uint32_t n,
                                                   const uint8_t* bits, bool comp, const G1A* table, uint32_t table_n,
                                                   bool& bad) {
  const uint32_t lane = threadIdx.x;
  G1J acc = jac_infinity<Fp>();
  uint32_t pending = 0;
  for (uint32_t base = 0; base < n; base += BLS_BLOCK) {
    const uint32_t j = base + lane;
    const bool sel = j < n && (!bits || committee_selects(bits, j, comp));
    const uint64_t mask = __ballot(sel);
    if (sel) ring[pending + __popcll(mask & ((1ull << lane) - 1ull))] = mem[j];
    pending += __popcll(mask);  // <= 63 + 64: the ring holds 128
    __syncthreads();
    if (pending >= BLS_BLOCK) {
      const uint32_t idx = ring[lane];
      const uint32_t rest = pending - BLS_BLOCK;
      const uint32_t carry = lane < rest ? ring[BLS_BLOCK + lane] : 0u;
      __syncthreads();
      if (lane < rest) ring[lane] = carry;
      pending = rest;
      if (idx >= table_n) bad = true;
      else acc = jac_add_aff(acc, table[idx]);
      __syncthreads();
    }
  }
  if (lane < pending) {
    const uint32_t idx = ring[lane];
    if (idx >= table_n) bad = true;
    else acc = jac_add_aff(acc, table[idx]);
  }
  part[lane] = acc;
  __syncthreads();
  for (uint32_t s = BLS_BLOCK / 2; s >= 1; s >>= 1) {
    if (lane < s) part[lane] = jac_add(part[lane], part[lane + s]);
    __syncthreads();
  }
}

// A committee set (b.bits_sets; bls_gpu_verify_committees) = the aggregate set whose index
// list is the committee's members at the set bits: one wavefront per set.  The lanes count
// the set bits, committee_use_complement picks the cheaper form -- the members whose bit is
// set, or the committee's total minus the members whose bit is clear -- and lane 0 writes
// what k_pk_agg writes.  The group law's edges are jac_add's: a complement equal to the
// total gives infinity, a duplicated member doubles.
__global__ __launch_bounds__(BLS_BLOCK) void k_pk_bits(PipeBufs b) {
  __shared__ G1J part[BLS_BLOCK];
  __shared__ uint32_t ring[2 * BLS_BLOCK];
  const uint32_t lane = threadIdx.x;
  const uint32_t i = b.bits_sets[blockIdx.x];
  const uint32_t ref = b.set_committee[i];
  const uint32_t g = committee_ref_group(ref), ci = committee_ref_index(ref);
  int32_t code = BLS_OK;
  G1J sum = jac_infinity<Fp>();
  if (g >= BLS_COMMITTEE_GROUPS || !b.cm_groups[g].offsets || ci >= b.cm_groups[g].n) {
    code = BLS_BAD_ENCODING;  // an unregistered group, an index past the group
  } else {
    const CommitteeGroupDev grp = b.cm_groups[g];
    const uint32_t beg = grp.offsets[ci], n = grp.offsets[ci + 1] - beg;
    const uint32_t boff = b.set_bits_off[i];
    const uint8_t* bits = b.bits + boff;
    code = committee_check_bits(bits, b.set_bits_off[i + 1] - boff, n);
    if (code == BLS_OK) {
      uint32_t c = 0;
      for (uint32_t base = 0; base < n; base += BLS_BLOCK) {
        const uint32_t j = base + lane;
        c += __popcll(__ballot(j < n && committee_bit(bits, j)));
      }
      if (c == 0) {
        code = BLS_EMPTY_AGGREGATE;
      } else {
        const bool comp = committee_use_complement(n, c);
        bool bad = false;
        committee_wave_sum(part, ring, grp.members + beg, n, bits, comp, b.pk_table, b.pk_table_n, bad);
        if (__any(bad)) code = BLS_BAD_ENCODING;
        if (lane == 0) {
          sum = part[0];
          if (comp) sum = jac_add(static_cast<const G1J*>(grp.totals)[ci], jac_neg(sum));
        }
      }
    }
  }
  if (lane == 0) {
    b.pk[i] = sum;
    b.pk_status[i] = code;
    if (b.pk_inf) b.pk_inf[i] = (code == BLS_OK && jac_is_inf(sum)) ? 1 : 0;
  }
}

hipError_t launch_k_pk_bits(const PipeBufs& b, hipStream_t s) {
  if (b.n_bits == 0) return hipSuccess;
  k_pk_bits<<<b.n_bits, BLS_BLOCK, 0, s>>>(b);
  return hipGetLastError();
}

// A span set (b.span_sets; bls_gpu_verify_spans) = the aggregate set whose index list is the
// members of its segments, concatenated, at the set bits of one field (bls/committee.hpp
// span_select_sum): one wavefront per set.
//   segments   lane k resolves segment k (at most BLS_SPAN_MAX_COMMITTEES = 64 = one lane
//              each): its group, its member range, its first bit (a prefix sum over LDS).
//   counts     c_k by k_pk_bits' ballot loop at the segment's bit offset;
//              committee_use_complement(n_k, c_k) segment by segment, kept as one 64-bit mask.
//   selection  a mainnet set is 64 segments of ~500 members, nearly all complemented with a
//              handful of clear bits each, so the selected positions of ALL segments go
//              through one compaction ring (committee_wave_sum's, an entry carrying its sign
//              as well: a complemented segment's clear-bit members are subtracted, the affine
//              point with y negated) that the lanes drain 64 at a time across segment
//              boundaries: at most ceil(S / 64) mixed additions per lane, S = sum_k min(c_k,
//              n_k - c_k), not one under-filled drain and one tree per segment.
//   totals     lane k takes the total of segment k if it is complemented, as the upper half
//              of the tree's input; the one tree then starts a level higher (128 entries).
// Every loop bound is uniform over the wavefront.  The group law's edges are jac_add's and
// jac_add_aff's: a committee repeated (P + P), a key taken once directly and once through a
// complement (P + (-P)), a total at infinity.
__global__ __launch_bounds__(BLS_BLOCK) void k_pk_span(PipeBufs b) {
  __shared__ G1J part[2 * BLS_BLOCK];
  __shared__ uint32_t ring[2 * BLS_BLOCK];
  __shared__ uint8_t ring_neg[2 * BLS_BLOCK];
  __shared__ uint32_t seg_n[BLS_BLOCK], seg_bit[BLS_BLOCK];
  __shared__ const uint32_t* seg_mem[BLS_BLOCK];
  const uint32_t lane = threadIdx.x;
  const uint32_t i = b.span_sets[blockIdx.x];
  const uint32_t sbeg = b.set_span_off[i];
  const uint32_t n_seg = b.set_span_off[i + 1] - sbeg;  // 1..64 (span_check_sets)
  int32_t code = BLS_OK;

  // ---- segments
  const G1J* my_total = nullptr;
  uint32_t my_n = 0;
  bool bad = false;
  if (lane < n_seg) {
    const uint32_t ref = b.span_refs[sbeg + lane];
    const uint32_t g = committee_ref_group(ref), ci = committee_ref_index(ref);
    if (g >= BLS_COMMITTEE_GROUPS || !b.cm_groups[g].offsets || ci >= b.cm_groups[g].n) {
      bad = true;  // an unregistered group, an index past the group
    } else {
      const CommitteeGroupDev grp = b.cm_groups[g];
      const uint32_t beg = grp.offsets[ci];
      my_n = grp.offsets[ci + 1] - beg;
      seg_mem[lane] = grp.members + beg;
      my_total = static_cast<const G1J*>(grp.totals) + ci;
    }
  }
  seg_n[lane] = my_n;
  __syncthreads();
  uint32_t my_bit = 0, total_n = 0;
  for (uint32_t k = 0; k < n_seg; ++k) {
    const uint32_t nk = seg_n[k];
    if (k < lane) my_bit += nk;
    total_n += nk;
  }
  seg_bit[lane] = my_bit;
  __syncthreads();
  if (__any(bad)) code = BLS_BAD_ENCODING;

  const uint32_t boff = b.set_bits_off[i];
  const uint8_t* bits = b.bits + boff;
  if (code == BLS_OK) code = span_check_bits(bits, b.set_bits_off[i + 1] - boff, total_n);

  G1J acc = jac_infinity<Fp>();
  G1J tot = jac_infinity<Fp>();
  if (code == BLS_OK) {
    // ---- counts
    uint64_t comp_mask = 0;
    uint32_t c_all = 0;
    for (uint32_t k = 0; k < n_seg; ++k) {
      const uint32_t n = seg_n[k], off = seg_bit[k];
      uint32_t c = 0;
      for (uint32_t base = 0; base < n; base += BLS_BLOCK) {
        const uint32_t j = base + lane;
        c += __popcll(__ballot(j < n && span_bit(bits, off, j)));
      }
      c_all += c;
      if (committee_use_complement(n, c)) comp_mask |= 1ull << k;
    }
    if (c_all == 0) {
      code = BLS_EMPTY_AGGREGATE;
    } else {
      // ---- selection: one ring over all segments
      uint32_t pending = 0;
      bool past = false;  // a member at or past the table (registration rules it out)
      for (uint32_t k = 0; k < n_seg; ++k) {
        const uint32_t n = seg_n[k], off = seg_bit[k];
        const uint32_t* mem = seg_mem[k];
        const bool comp = (comp_mask >> k) & 1ull;
        for (uint32_t base = 0; base < n; base += BLS_BLOCK) {
          const uint32_t j = base + lane;
          const bool sel = j < n && span_selects(bits, off, j, comp);
          const uint64_t mask = __ballot(sel);
          if (sel) {
            const uint32_t at = pending + __popcll(mask & ((1ull << lane) - 1ull));
            ring[at] = mem[j];
            ring_neg[at] = comp ? 1 : 0;
          }
          pending += __popcll(mask);  // <= 63 + 64: the ring holds 128
          __syncthreads();
          if (pending >= BLS_BLOCK) {
            const uint32_t idx = ring[lane];
            const bool neg = ring_neg[lane] != 0;
            const uint32_t rest = pending - BLS_BLOCK;
            const uint32_t carry = lane < rest ? ring[BLS_BLOCK + lane] : 0u;
            const uint8_t carry_neg = lane < rest ? ring_neg[BLS_BLOCK + lane] : (uint8_t)0;
            __syncthreads();
            if (lane < rest) {
              ring[lane] = carry;
              ring_neg[lane] = carry_neg;
            }
            pending = rest;
            if (idx >= b.pk_table_n) {
              past = true;
            } else {
              G1A q = b.pk_table[idx];
              if (neg) q.y = fp_neg(q.y);
              acc = jac_add_aff(acc, q);
            }
            __syncthreads();
          }
        }
      }
      if (lane < pending) {
        const uint32_t idx = ring[lane];
        if (idx >= b.pk_table_n) {
          past = true;
        } else {
          G1A q = b.pk_table[idx];
          if (ring_neg[lane]) q.y = fp_neg(q.y);
          acc = jac_add_aff(acc, q);
        }
      }
      if (__any(past)) code = BLS_BAD_ENCODING;
      // ---- totals
      if (lane < n_seg && ((comp_mask >> lane) & 1ull)) tot = *my_total;
    }
  }
  // ---- one tree over the lanes' sums and the complemented segments' totals
  part[lane] = acc;
  part[BLS_BLOCK + lane] = tot;
  __syncthreads();
  for (uint32_t s = BLS_BLOCK; s >= 1; s >>= 1) {
    if (lane < s) part[lane] = jac_add(part[lane], part[lane + s]);
    __syncthreads();
  }
  if (lane == 0) {
    const G1J sum = code == BLS_OK ? part[0] : jac_infinity<Fp>();
    b.pk[i] = sum;
    b.pk_status[i] = code;
    if (b.pk_inf) b.pk_inf[i] = (code == BLS_OK && jac_is_inf(sum)) ? 1 : 0;
  }
}

hipError_t launch_k_pk_span(const PipeBufs& b, hipStream_t s) {
  if (b.n_span == 0) return hipSuccess;
  k_pk_span<<<b.n_span, BLS_BLOCK, 0, s>>>(b);
  return hipGetLastError();
}

// Registration of a committee group (bls_gpu_set_committee_group): committee blockIdx.x's
// total, the sum over all of its members with multiplicity.
__global__ __launch_bounds__(BLS_BLOCK) void k_committee_totals(CommitteeGroupDev grp, G1J* totals, const G1A* table,
                                                                uint32_t table_n) {
  __shared__ G1J part[BLS_BLOCK];
  __shared__ uint32_t ring[2 * BLS_BLOCK];
  const uint32_t ci = blockIdx.x;
  const uint32_t beg = grp.offsets[ci], n = grp.offsets[ci + 1] - beg;
  bool bad = false;
  committee_wave_sum(part, ring, grp.members + beg, n, nullptr, false, table, table_n, bad);
  if (threadIdx.x == 0) totals[ci] = part[0];
}

hipError_t launch_k_committee_totals(const CommitteeGroupDev& grp, G1J* totals, const G1A* table, uint32_t table_n,
                                     hipStream_t s) {
  if (grp.n == 0) return hipSuccess;
  k_committee_totals<<<grp.n, BLS_BLOCK, 0, s>>>(grp, totals, table, table_n);
  return hipGetLastError();
}

__global__ __launch_bounds__(BLS_BLOCK) void k_aggregate(PipeBufs b, uint8_t* out96) {
  uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  stage_pk(b, i);
  if (i < b.n_sets) g1_serialize96(jac_to_aff(b.pk[i]), out96 + 96ull * i);
}

__global__ __launch_bounds__(BLS_BLOCK) void k_load_pubkeys(const uint8_t* pks, uint32_t n, uint32_t pk_len,
                                                            G1A* out, int32_t* codes) {
  uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i >= n) return;
  G1A a;
  int32_t c = pk_len == 48 ? g1_decompress48(pks + 48ull * i, a) : g1_deserialize96(pks + 96ull * i, a);
  if (c != BLS_OK) {
    a.inf = true;
    a.x = fp_zero();
    a.y = fp_zero();
  }
  out[i] = a;
  codes[i] = c;
}

// Comb rows of n freshly loaded table keys (curve.hpp g1_comb_build), one lane per key:
// rows[G1_COMB_WORDS * i ..] and ok[i] for key keys[i]; tmp holds the lane's 15 Jacobian
// entries until they are affine (15 n G1J of workspace, not a 2 KB private frame).  Two
// wavefronts per SIMD at the most, so its scratch reservation per queue stays under the
// verify path's deepest kernel (lodestar_amd/build.py scratch_per_queue).
__global__ __launch_bounds__(BLS_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_comb_build(
    const G1A* keys, uint32_t n, G1J* tmp, Fp* rows, uint8_t* ok) {
  const uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const G1A p = keys[i];
  ok[i] = g1_comb_build(p, tmp + (size_t)G1_COMB_ROWS * i, rows + (size_t)G1_COMB_WORDS * i) ? 1 : 0;
}

hipError_t launch_k_comb_build(const G1A* keys, uint32_t n, G1J* tmp, Fp* rows, uint8_t* ok, hipStream_t s) {
  if (n == 0) return hipSuccess;
  k_comb_build<<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(keys, n, tmp, rows, ok);
  return hipGetLastError();
}

// KeyValidate (blst PublicKey.fromBytes(bytes, validate=true) [ext], as the deposit
// path uses it, block/processDeposit.ts:56-65): decode, reject infinity, G1 subgroup.
__global__ __launch_bounds__(BLS_BLOCK) void k_validate_pubkeys(const uint8_t* pks, uint32_t n, uint32_t pk_len,
                                                                int32_t* codes) {
  uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i >= n) return;
  G1A a;
  int32_t c = pk_len == 48 ? g1_decompress48(pks + 48ull * i, a) : g1_deserialize96(pks + 96ull * i, a);
  if (c == BLS_OK && a.inf) c = BLS_PK_IS_INFINITY;
  if (c == BLS_OK && !g1_in_subgroup(a)) c = BLS_POINT_NOT_IN_GROUP;
  codes[i] = c;
}

hipError_t launch_k_validate_pubkeys(const uint8_t* pks, uint32_t n, uint32_t pk_len, int32_t* codes, hipStream_t s) {
  k_validate_pubkeys<<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(pks, n, pk_len, codes);
  return hipGetLastError();
}

// Per-request status; also mirrors the statuses and the exact-path count into the
// context's host-mapped result area (read by the host after the stream syncs, no D2H
// copy blits).
__global__ __launch_bounds__(BLS_BLOCK) void k_status(PipeBufs b) {
  BLS_TAIL_PRIO();
  const uint32_t r = blockIdx.x * BLS_BLOCK + threadIdx.x;
  stage_req_status(b, r);
  if (b.req_status_host && r < b.n_reqs) b.req_status_host[r] = b.req_status[r];
  if (r == 0 && b.flag_count_host) *b.flag_count_host = b.n_sets ? *b.flag_count : 0u;
}

hipError_t launch_k_pk(const PipeBufs& b, hipStream_t s) {
  k_pk<<<bls_grid_for(b.n_sets), BLS_BLOCK, 0, s>>>(b);
  return hipGetLastError();
}
hipError_t launch_k_aggregate(const PipeBufs& b, uint8_t* out96, hipStream_t s) {
  k_aggregate<<<bls_grid_for(b.n_sets), BLS_BLOCK, 0, s>>>(b, out96);
  return hipGetLastError();
}
hipError_t launch_k_load_pubkeys(const uint8_t* pks, uint32_t n, uint32_t pk_len, G1A* out, int32_t* codes,
                                 hipStream_t s) {
  k_load_pubkeys<<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(pks, n, pk_len, out, codes);
  return hipGetLastError();
}
hipError_t launch_k_status(const PipeBufs& b, hipStream_t s) {
  k_status<<<bls_grid_for(b.n_reqs), BLS_BLOCK, 0, s>>>(b);
  return hipGetLastError();
}
