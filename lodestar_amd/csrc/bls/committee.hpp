// Committee groups: the member lists of an epoch's shuffling or of a sync committee, kept on
// the device with each committee's total key, so that an aggregate set can arrive as
// (committee, participation bits) instead of an index list (bls_gpu_set_committee_group,
// bls_gpu_verify_committees; kernels/k_pk.hip k_pk_bits).
//
//   rules       what a bitfield selects, shared by the kernel, the verifiers' routing weight
//               and the host test: the SSZ bit order, the length and padding checks, and
//               committee_use_complement -- the one place that decides between summing the
//               members whose bit is set and total - (the members whose bit is clear).
//               Then the same for a span, one field over several committees
//               (bls_gpu_verify_spans; k_pk_span): the bit accessor at a bit offset, the
//               checks over the sum of the sizes, span_weight and span_select_sum.
//   group       one device allocation: member_offsets (n + 1), members, then one G1J total
//               per committee, each part 256-byte aligned.  Registered and replaced
//               wholesale; the slot changes only after the new totals are complete.
//   slots       BLS_COMMITTEE_GROUPS groups per context, with their byte accounting.  Device
//               memory sits behind PkMem, so this file also compiles for the CPU
//               (tests/native/committee_host.cpp).
// The groups belong to the context.  Holding them in the shared PkTable generation, so that
// the contexts of one device register a shuffling once, is a follow-up: until then a host
// with several contexts registers a group through each of them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/lodestar_bls.h"
#include "pk_table.hpp"

#ifndef BLS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BLS_HD __host__ __device__ __forceinline__
#else
#define BLS_HD static inline
#endif
#endif

namespace bls {

// ---- rules ---------------------------------------------------------------------------

// member j of a committee = bit (j & 7) of byte j >> 3 (SSZ Bitvector order; a Bitlist's
// delimiter bit is not part of the field)
BLS_HD bool committee_bit(const uint8_t* bits, uint32_t j) { return (bits[j >> 3] >> (j & 7u)) & 1u; }
BLS_HD uint32_t committee_bits_bytes(uint32_t n_members) { return (n_members + 7u) >> 3; }
// the bits of the last byte at or past member n (0 when n fills its last byte)
BLS_HD uint32_t committee_padding_mask(uint32_t n_members) {
  return (n_members & 7u) ? (0xFFu << (n_members & 7u)) & 0xFFu : 0u;
}

// Of n members, c have their bit set.  The direct sum costs c - 1 additions (c into an
// accumulator at infinity); the complement n - c of them and one more for total + (-sum).
// Complement exactly when that is strictly fewer.
BLS_HD bool committee_use_complement(uint32_t n, uint32_t c) { return (uint64_t)n - c + 1u < (uint64_t)c; }
// whether position j is summed: the set bits directly, the clear ones for the complement
BLS_HD bool committee_selects(const uint8_t* bits, uint32_t j, bool complement) {
  return committee_bit(bits, j) != complement;
}
// keys a committee set costs its device (the verifiers' routing weight, in place of k)
BLS_HD uint32_t committee_weight(uint32_t n, uint32_t c) { return 1u + (c < n - c ? c : n - c); }

// BLS_CODE_OK, or BLS_CODE_BAD_ENCODING for a field of the wrong length or with a padding
// bit set (a set bit at or past the member count)
BLS_HD int32_t committee_check_bits(const uint8_t* bits, uint32_t n_bytes, uint32_t n_members) {
  if (n_bytes != committee_bits_bytes(n_members)) return BLS_CODE_BAD_ENCODING;
  const uint32_t pad = committee_padding_mask(n_members);
  if (pad && (bits[n_bytes - 1] & pad)) return BLS_CODE_BAD_ENCODING;
  return BLS_CODE_OK;
}

BLS_HD uint32_t committee_popcount(const uint8_t* bits, uint32_t n_members) {
  uint32_t c = 0;
  for (uint32_t j = 0; j < n_members; ++j) c += committee_bit(bits, j) ? 1u : 0u;
  return c;
}

// One lane's statement of what k_pk_bits computes for a field that passed
// committee_check_bits: the sum over the set bits, taken directly or as total - (the sum
// over the clear bits).  at(member), add(a, b), neg(a) and zero are the group's; the host
// test runs it over integers, where both branches must give the direct sum.
template <class P, class At, class Add, class Neg>
BLS_HD P committee_select_sum(const uint32_t* members, uint32_t n, const uint8_t* bits, const P& total, const P& zero,
                              bool allow_complement, At at, Add add, Neg neg) {
  const bool comp = allow_complement && committee_use_complement(n, committee_popcount(bits, n));
  P acc = zero;
  for (uint32_t j = 0; j < n; ++j)
    if (committee_selects(bits, j, comp)) acc = add(acc, at(members[j]));
  return comp ? add(total, neg(acc)) : acc;
}

// ---- rules of a span: several committees under one field ----------------------------------
//
// A span (bls_span_sets, bls_gpu_verify_spans; kernels/k_pk.hip k_pk_span) is the members of
// its segments -- registered committees, repeats and several groups allowed -- concatenated
// in order, under one field that runs over the concatenation without a break: segment k of
// sizes n_0, n_1, ... starts at bit n_0 + ... + n_{k-1}, so every segment after the first
// may start mid-byte.  This is Electra's Attestation (EIP-7549): committee_bits picks the
// segments, aggregation_bits is the field.

// bit j of the segment that starts at bit bit_off of the field
BLS_HD bool span_bit(const uint8_t* bits, uint32_t bit_off, uint32_t j) { return committee_bit(bits, bit_off + j); }
BLS_HD bool span_selects(const uint8_t* bits, uint32_t bit_off, uint32_t j, bool complement) {
  return span_bit(bits, bit_off, j) != complement;
}
BLS_HD uint32_t span_popcount(const uint8_t* bits, uint32_t bit_off, uint32_t n_members) {
  uint32_t c = 0;
  for (uint32_t j = 0; j < n_members; ++j) c += span_bit(bits, bit_off, j) ? 1u : 0u;
  return c;
}
// the members of a span (64 segments of BLS_COMMITTEE_MAX_MEMBERS: 2^23, no wrap)
BLS_HD uint32_t span_members(const uint32_t* seg_n, uint32_t n_seg) {
  uint32_t total = 0;
  for (uint32_t k = 0; k < n_seg; ++k) total += seg_n[k];
  return total;
}
// the length and padding check of a span's field: committee_check_bits over the sum of the
// segments' sizes (only the last segment's end is followed by padding)
BLS_HD int32_t span_check_bits(const uint8_t* bits, uint32_t n_bytes, uint32_t total_members) {
  return committee_check_bits(bits, n_bytes, total_members);
}
// keys a span set costs its device: each segment by itself, as committee_weight has it
BLS_HD uint32_t span_weight(const uint32_t* seg_n, const uint32_t* seg_c, uint32_t n_seg) {
  uint32_t w = 0;
  for (uint32_t k = 0; k < n_seg; ++k) w += committee_weight(seg_n[k], seg_c[k]);
  return w;
}

// One lane's statement of what k_pk_span computes for a field that passed span_check_bits:
// the sum over the set bits of the concatenation, each segment taken by itself either
// directly or as its total minus the members whose bit is clear, by
// committee_use_complement(n_k, c_k).  seg_members[k] are segment k's n_k = seg_n[k] members
// and seg_total[k] its total; at / add / neg / zero as in committee_select_sum.
template <class P, class At, class Add, class Neg>
BLS_HD P span_select_sum(const uint32_t* const* seg_members, const uint32_t* seg_n, const P* seg_total, uint32_t n_seg,
                         const uint8_t* bits, const P& zero, bool allow_complement, At at, Add add, Neg neg) {
  P acc = zero;
  uint32_t bit_off = 0;
  for (uint32_t k = 0; k < n_seg; ++k) {
    const uint32_t n = seg_n[k];
    const bool comp = allow_complement && committee_use_complement(n, span_popcount(bits, bit_off, n));
    for (uint32_t j = 0; j < n; ++j)
      if (span_selects(bits, bit_off, j, comp))
        acc = add(acc, comp ? neg(at(seg_members[k][j])) : at(seg_members[k][j]));
    if (comp) acc = add(acc, seg_total[k]);
    bit_off += n;
  }
  return acc;
}

// ---- a group as the kernels see it -----------------------------------------------------

struct CommitteeGroupDev {
  const uint32_t* offsets;  // n + 1 into members (nullptr: the group is not registered)
  const uint32_t* members;  // table indices, all below the table's size at registration
  const void* totals;       // n G1J: each committee's sum over all members, with multiplicity
  uint32_t n;
  uint32_t pad_;
};

BLS_HD uint32_t committee_ref_group(uint32_t ref) { return ref >> 24; }
BLS_HD uint32_t committee_ref_index(uint32_t ref) { return ref & 0xFFFFFFu; }

// ---- registration arguments --------------------------------------------------------------

// 0, or -2 with a message naming the committee: group past the slots, offsets that do not
// start at 0 or run backwards, an empty committee, one past the cap, a member at or past
// the table's size
static inline int committee_check_group(uint32_t group, uint32_t n, const uint32_t* member_offsets,
                                        const uint32_t* members, uint32_t table_n, char* err, size_t err_len) {
  if (group >= BLS_COMMITTEE_GROUPS) {
    snprintf(err, err_len, "committee group %u: only groups 0..%u exist", group, BLS_COMMITTEE_GROUPS - 1u);
    return -2;
  }
  if (n == 0) return 0;
  if (n > 0x1000000u) {
    snprintf(err, err_len, "committee group %u: %u committees, a reference indexes 2^24", group, n);
    return -2;
  }
  if (!member_offsets || !members) {
    snprintf(err, err_len, "committee group %u: member_offsets or members missing", group);
    return -2;
  }
  if (member_offsets[0] != 0) {
    snprintf(err, err_len, "committee group %u: member_offsets[0] != 0", group);
    return -2;
  }
  for (uint32_t c = 0; c < n; ++c) {
    const uint32_t beg = member_offsets[c], end = member_offsets[c + 1];
    if (end < beg) {
      snprintf(err, err_len, "committee group %u: member_offsets not monotone at committee %u", group, c);
      return -2;
    }
    if (end == beg) {
      snprintf(err, err_len, "committee group %u: committee %u is empty", group, c);
      return -2;
    }
    if (end - beg > BLS_COMMITTEE_MAX_MEMBERS) {
      snprintf(err, err_len, "committee group %u: committee %u has %u members, the cap is %u", group, c, end - beg,
               BLS_COMMITTEE_MAX_MEMBERS);
      return -2;
    }
    for (uint32_t k = beg; k < end; ++k)
      if (members[k] >= table_n) {
        snprintf(err, err_len, "committee group %u: committee %u member %u is table index %u, the table holds %u keys",
                 group, c, k - beg, members[k], table_n);
        return -2;
      }
  }
  return 0;
}

// 0, or -2 with a message: the arrays of a bls_committee_sets against the call's sets
static inline int committee_check_sets(const bls_committee_sets* cs, uint32_t n_sets, const uint32_t* set_pk_offsets,
                                       char* err, size_t err_len) {
  if (!cs || (n_sets && (!cs->set_committee || !cs->set_bits_off))) {
    snprintf(err, err_len, "committee sets: set_committee or set_bits_off missing");
    return -2;
  }
  if (n_sets == 0) return 0;
  if (cs->set_bits_off[0] != 0) {
    snprintf(err, err_len, "committee sets: set_bits_off[0] != 0");
    return -2;
  }
  for (uint32_t i = 0; i < n_sets; ++i) {
    const uint32_t beg = cs->set_bits_off[i], end = cs->set_bits_off[i + 1];
    if (end < beg) {
      snprintf(err, err_len, "committee sets: set_bits_off not monotone at set %u", i);
      return -2;
    }
    if (cs->set_committee[i] == BLS_SET_NO_COMMITTEE) {
      if (end != beg) {
        snprintf(err, err_len, "committee sets: set %u names no committee and carries %u bytes of bits", i, end - beg);
        return -2;
      }
    } else if (set_pk_offsets && set_pk_offsets[i + 1] != set_pk_offsets[i]) {
      snprintf(err, err_len, "committee sets: set %u names a committee and carries an index list", i);
      return -2;
    }
  }
  if (cs->set_bits_off[n_sets] && !cs->bits) {
    snprintf(err, err_len, "committee sets: bits missing");
    return -2;
  }
  return 0;
}

// 0, or -2 with a message naming the set: the arrays of a bls_span_sets against the call's
// sets.  in_batch: the sets belong to a bls_batch (bls_gpu_verify_spans), which must carry
// table indices (set_pk_offsets; a raw-key batch is refused) and may mix index-list sets in;
// otherwise (bls_gpu_aggregate_spans) every set needs at least one segment.
static inline int span_check_sets(const bls_span_sets* ss, uint32_t n_sets, bool in_batch,
                                  const uint32_t* set_pk_offsets, char* err, size_t err_len) {
  if (!ss || (n_sets && (!ss->set_span_off || !ss->set_bits_off))) {
    snprintf(err, err_len, "span sets: set_span_off or set_bits_off missing");
    return -2;
  }
  if (n_sets == 0) return 0;
  if (in_batch && !set_pk_offsets) {
    snprintf(err, err_len, "span sets: the batch must carry table indices (set_pk_offsets), not raw keys");
    return -2;
  }
  if (ss->set_span_off[0] != 0 || ss->set_bits_off[0] != 0) {
    snprintf(err, err_len, "span sets: %s[0] != 0 (set 0)", ss->set_span_off[0] ? "set_span_off" : "set_bits_off");
    return -2;
  }
  for (uint32_t i = 0; i < n_sets; ++i) {
    const uint32_t sbeg = ss->set_span_off[i], send = ss->set_span_off[i + 1];
    const uint32_t beg = ss->set_bits_off[i], end = ss->set_bits_off[i + 1];
    if (send < sbeg) {
      snprintf(err, err_len, "span sets: set_span_off not monotone at set %u", i);
      return -2;
    }
    if (end < beg) {
      snprintf(err, err_len, "span sets: set_bits_off not monotone at set %u", i);
      return -2;
    }
    if (send - sbeg > BLS_SPAN_MAX_COMMITTEES) {
      snprintf(err, err_len, "span sets: set %u has %u segments, the cap is %u", i, send - sbeg,
               BLS_SPAN_MAX_COMMITTEES);
      return -2;
    }
    if (send == sbeg) {
      if (!in_batch) {
        snprintf(err, err_len, "span sets: set %u has no segment", i);
        return -2;
      }
      if (end != beg) {
        snprintf(err, err_len, "span sets: set %u has no segment and carries %u bytes of bits", i, end - beg);
        return -2;
      }
    } else if (set_pk_offsets && set_pk_offsets[i + 1] != set_pk_offsets[i]) {
      snprintf(err, err_len, "span sets: set %u is a span and carries an index list", i);
      return -2;
    }
  }
  if (ss->set_span_off[n_sets] && !ss->span_refs) {
    snprintf(err, err_len, "span sets: span_refs missing");
    return -2;
  }
  if (ss->set_bits_off[n_sets] && !ss->bits) {
    snprintf(err, err_len, "span sets: bits missing");
    return -2;
  }
  return 0;
}

// ---- the slots -----------------------------------------------------------------------

struct CommitteeLayout {
  size_t offsets_at, members_at, totals_at, bytes;
};
static inline CommitteeLayout committee_layout(uint32_t n, uint32_t n_members, size_t total_bytes) {
  const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  CommitteeLayout l;
  l.offsets_at = 0;
  l.members_at = up(sizeof(uint32_t) * ((size_t)n + 1));
  l.totals_at = l.members_at + up(sizeof(uint32_t) * (size_t)n_members);
  l.bytes = l.totals_at + total_bytes * (size_t)n;
  return l;
}

class CommitteeSlots {
 public:
  // total_bytes: one committee's total (sizeof(G1J) on the device)
  CommitteeSlots(const PkMem* mem, size_t total_bytes) : mem_(mem), total_(total_bytes) {
    for (Slot& s : slot_) s = Slot{};
  }
  CommitteeSlots(const CommitteeSlots&) = delete;
  CommitteeSlots& operator=(const CommitteeSlots&) = delete;
  ~CommitteeSlots() { clear(); }

  // Replace group `group` (n == 0: drop it).  The arguments passed committee_check_group.
  // upload(dst, src, bytes) copies host memory to the new allocation and totals(view)
  // fills view.totals from the other two parts; both wait for the device and return false
  // on a failure.  0 done; -1 with *what naming the step, the slot as it was.
  template <class Upload, class Totals>
  int set(uint32_t group, uint32_t n, const uint32_t* member_offsets, const uint32_t* members, Upload&& upload,
          Totals&& totals, const char** what) {
    Slot fresh{};
    if (n) {
      const uint32_t n_members = member_offsets[n];
      const CommitteeLayout l = committee_layout(n, n_members, total_);
      uint8_t* p = (uint8_t*)mem_->alloc(l.bytes);
      if (!p) return fail(what, "committee group allocation");
      fresh.p = p;
      fresh.bytes = l.bytes;
      fresh.n = n;
      fresh.n_members = n_members;
      fresh.view = view_of(p, l, n);
      if (!upload(p + l.offsets_at, member_offsets, sizeof(uint32_t) * ((size_t)n + 1)) ||
          !upload(p + l.members_at, members, sizeof(uint32_t) * (size_t)n_members)) {
        mem_->free(p);
        return fail(what, "committee group copy");
      }
      if (!totals(fresh.view)) {
        mem_->free(p);
        return fail(what, "committee totals");
      }
    }
    Slot old = slot_[group];
    slot_[group] = fresh;
    if (old.p) mem_->free(old.p);
    return 0;
  }

  void clear() {
    for (Slot& s : slot_) {
      if (s.p) mem_->free(s.p);
      s = Slot{};
    }
  }

  bls_committee_info info(uint32_t group) const {
    const Slot& s = slot_[group];
    return bls_committee_info{s.n, s.n_members, (uint64_t)s.bytes};
  }
  uint64_t device_bytes() const {
    uint64_t b = 0;
    for (const Slot& s : slot_) b += s.bytes;
    return b;
  }
  // what the kernels read: BLS_COMMITTEE_GROUPS views (offsets == nullptr: not registered)
  void views(CommitteeGroupDev out[BLS_COMMITTEE_GROUPS]) const {
    for (uint32_t g = 0; g < BLS_COMMITTEE_GROUPS; ++g) out[g] = slot_[g].view;
  }

 private:
  struct Slot {
    uint8_t* p;
    size_t bytes;
    uint32_t n, n_members;
    CommitteeGroupDev view;
  };
  static CommitteeGroupDev view_of(uint8_t* p, const CommitteeLayout& l, uint32_t n) {
    return CommitteeGroupDev{(const uint32_t*)(p + l.offsets_at), (const uint32_t*)(p + l.members_at),
                             (const void*)(p + l.totals_at), n, 0u};
  }
  static int fail(const char** what, const char* msg) {
    if (what) *what = msg;
    return -1;
  }

  const PkMem* const mem_;
  const size_t total_;
  Slot slot_[BLS_COMMITTEE_GROUPS];
};

}  // namespace bls
