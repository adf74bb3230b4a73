"""Spans (aggregate sets over several committees under one field, EIP-7549) without a GPU: the
span rules of bls/committee.hpp -- what bls_gpu_verify_spans, bls_gpu_aggregate_spans,
k_pk_span and the routing weight share -- compiled for the host (tests/native/span_host.cpp).
The program checks the bit accessor at a bit offset, the length and padding check at sums of
8, 9, 16, 17, 64 and 65 members however they are cut into segments, span_weight, every -2
case of span_check_sets with its message, and span_select_sum over integers standing in for
points: the plain sum over the set bits for every combination of per-segment patterns, read
with sum_k min(c_k, n_k - c_k) member reads, the complement taken exactly when
committee_use_complement says so.  Once plain and once under AddressSanitizer + UBSan, each as
a stand-alone program.  Then pack_requests of span dicts: offsets, refs and bits bit-exact."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from lodestar_amd._abi import COMMITTEE_REF
from lodestar_amd.build import build_span_host
from lodestar_amd.native import pack_requests
from lodestar_amd.verifier import committee_weight_keys, span_weight_keys
from tests._spans import concat_bits, span_expand


def _self_check(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 20000, out.stdout[-500:]


def test_span_rules():
    _self_check(build_span_host(verbose=False))


def test_under_address_sanitizer(tmp_path):
    """the same program with -fsanitize=address,undefined: any report makes it exit non-zero"""
    exe = build_span_host(verbose=False, out=tmp_path / "span_host_asan",
                          extra=["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                 "-fno-omit-frame-pointer"])
    _self_check(exe)


def test_span_weight_keys():
    assert span_weight_keys([512], [507]) == committee_weight_keys(512, 507) == 6
    assert span_weight_keys([512, 8, 9], [5, 4, 0]) == 6 + 5 + 1
    assert span_weight_keys([500] * 64, [495] * 64) == 64 * 6
    assert span_weight_keys([], []) == 0


def test_concat_bits_starts_segments_mid_byte():
    # 7 members all set, then 9 members with the first and the last set: bits 0..6, 7 and 15
    assert concat_bits([(7, range(7)), (9, [0, 8])]) == bytes([0xFF, 0x80])
    assert concat_bits([(1, [0]), (1, []), (1, [0])]) == bytes([0b101])
    assert concat_bits([(9, []), (63, [0]), (65, [64])]) == bytes([0, 0x02] + [0] * 15 + [0x01])
    members = [[10, 11, 12], [20, 21], [10, 11, 12]]
    assert span_expand(members, concat_bits([(3, [1]), (2, [0, 1]), (3, [0, 2])])) == [11, 20, 21, 10, 12]


M, S = bytes(range(32)), bytes(96)


def test_pack_requests_span_dicts():
    """offsets, refs and bits as bls_span_sets wants them; beside a span, a {"committee": ...}
    dict is a one-segment span and an index-list set has empty ranges"""
    f0 = concat_bits([(7, [0, 6]), (9, [0, 8])])          # 2 bytes, the second segment from bit 7
    f1 = bytes([0x1F, 0x01])                               # a 9-member committee
    f2 = concat_bits([(1, [0]), (1, []), (1, [0])])        # 1 byte
    reqs = [
        (True, [{"committees": [(0, 1), (0, 3)], "bits": f0, "message": M, "signature": S}]),
        (False, [([4, 5, 6], M, S), {"committee": (2, 3), "bits": f1, "message": M, "signature": S}]),
        (True, [{"committees": ((1, 0), (1, 0), (7, 0xFFFFFF)), "bits": f2, "message": M, "signature": S[:95]},
                ([9], M, S)]),
    ]
    pb = pack_requests(reqs, seed=M)
    assert pb.set_committee is None and pb.set_span_off is not None
    assert pb.set_span_off.dtype == pb.span_refs.dtype == pb.set_bits_off.dtype == np.uint32 and pb.bits.dtype == np.uint8
    assert list(pb.req_set_offsets) == [0, 1, 3, 5] and list(pb.req_batchable) == [1, 0, 1]
    assert list(pb.set_span_off) == [0, 2, 2, 3, 6, 6]
    assert list(pb.span_refs) == [COMMITTEE_REF(0, 1), COMMITTEE_REF(0, 3), COMMITTEE_REF(2, 3), COMMITTEE_REF(1, 0),
                                  COMMITTEE_REF(1, 0), 0x07FFFFFF]
    assert list(pb.set_bits_off) == [0, 2, 2, 4, 5, 5]
    assert pb.bits.tobytes() == f0 + f1 + f2
    assert list(pb.set_pk_offsets) == [0, 0, 3, 3, 3, 4] and list(pb.pk_indices) == [4, 5, 6, 9]
    assert list(pb.signature_lens) == [96, 96, 96, 95, 96]


def test_pack_requests_without_a_span_is_unchanged():
    """committee dicts alone keep the bls_committee_sets form; index lists alone carry neither"""
    pb = pack_requests([(True, [{"committee": (2, 3), "bits": b"\x03", "message": M, "signature": S}, ([1], M, S)])])
    assert pb.set_span_off is None and pb.span_refs is None
    assert list(pb.set_committee) == [COMMITTEE_REF(2, 3), 0xFFFFFFFF] and list(pb.set_bits_off) == [0, 1, 1]
    pb = pack_requests([(True, [([1], M, S)])])
    assert pb.set_span_off is None and pb.set_committee is None and pb.bits is None


def test_pack_requests_rejects_what_cannot_be_a_span():
    with pytest.raises(ValueError, match="at least one committee"):
        pack_requests([(True, [{"committees": [], "bits": b"", "message": M, "signature": S}])])
    with pytest.raises(ValueError, match="mixed raw / table"):
        pack_requests([(True, [(bytes(96), M, S), {"committees": [(0, 0)], "bits": b"\x01", "message": M, "signature": S}])])
