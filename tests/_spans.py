"""Shared by the span tests (tests/test_span_cpu.py, tests/test_gpu_committee_spans.py,
tests/test_verifier_spans.py, tests/test_napi_spans.py): a span's field built segment by
segment, its expanded index list, the per-segment patterns, and the key table and committee
groups of the GPU tests -- the 109-key table and the size sweep of tests/test_gpu_committees.py
(committees of 1, 7, 8, 9, 63, 64, 65 and 129 members drawn with the same seed), and a group of
structured committees for the group law's edges."""
from __future__ import annotations

import random

from oracle import bls_oracle as O
from tests import _groupedge as ge

SIZES = (1, 7, 8, 9, 63, 64, 65, 129)
EXTRA_BASE = 41  # interop key 32 + j at table index 41 + j, j < 68
POOL = list(range(32)) + list(range(EXTRA_BASE, EXTRA_BASE + 68))  # the 100 distinct interop keys
G_SIZES, G_STRUCT, G_SWAP, G_NEVER = 0, 1, 2, 5

# group G_STRUCT
C_POS = [0, 1, 2, 3, 4, 5, 6, 7]                       # sk_0 .. sk_7
C_NEG = [ge.neg(j) for j in range(8)]                  # r - sk_0 .. r - sk_7: C_POS + C_NEG is infinity
C_PAIR = [3, ge.neg(3)]                                # a total at infinity
C_SHARE_A = [10, 11, 12, 13, 14, 15, 16, 17, 18]       # key 12 is member 2 here ...
C_SHARE_B = [20, 21, 22, 12, 23, 24, 25, 26, 27]       # ... and member 3 here
STRUCT = [C_POS, C_NEG, C_PAIR, C_SHARE_A, C_SHARE_B]
S_POS, S_NEG, S_PAIR, S_SHARE_A, S_SHARE_B = range(5)


def _size_committees():
    rng = random.Random(20261020)
    return [rng.sample(POOL, n) if n <= len(POOL) else POOL + rng.sample(POOL, n - len(POOL)) for n in SIZES]


SIZE_COMMITTEES = _size_committees()
GROUPS = {G_SIZES: SIZE_COMMITTEES, G_STRUCT: STRUCT}


def size_ref(n: int):
    """(group, index) of the size sweep's committee of n members"""
    return (G_SIZES, SIZES.index(n))


def members_of(refs):
    return [GROUPS[g][i] for g, i in refs]


def table_sk(i: int) -> int:
    return O.interop_secret_key(32 + i - EXTRA_BASE) if i >= EXTRA_BASE else ge.table_sk(i)


def table_keys(golden) -> list[bytes]:
    keys = ge.table_keys(golden) + [bytes.fromhex(h) for h in golden["kat2_interop_pubkeys"][32:100]]
    assert len(keys) == 109
    return keys


def concat_bits(segs) -> bytes:
    """segs: [(n_members, positions set within the segment)].  One field over the concatenation,
    SSZ order (bit j = bit j & 7 of byte j >> 3), no delimiter: segment k starts at the bit where
    segment k - 1 ended, mid-byte or not."""
    total = sum(n for n, _ in segs)
    b = bytearray((total + 7) // 8)
    off = 0
    for n, pos in segs:
        for j in pos:
            assert 0 <= j < n
            b[(off + j) >> 3] |= 1 << ((off + j) & 7)
        off += n
    return bytes(b)


def span_expand(seg_members, bits: bytes):
    """the index list a span stands for: the segments' members, concatenated, at the set bits"""
    flat = [m for seg in seg_members for m in seg]
    return [m for j, m in enumerate(flat) if (bits[j >> 3] >> (j & 7)) & 1]


PATTERNS = ("all", "all_but_first", "all_but_last", "first_only", "last_only", "none", "half")


def pattern(name: str, n: int):
    return {
        "all": range(n),
        "all_but_first": range(1, n),
        "all_but_last": range(n - 1),
        "first_only": [0],
        "last_only": [n - 1],
        "none": [],
        "half": range(n // 2),
    }[name]


def use_complement(n: int, c: int) -> bool:
    """committee_use_complement (bls/committee.hpp)"""
    return n - c + 1 < c


class SpanCtx:
    """A GpuContext of its own with the table and both groups registered"""

    def __init__(self, golden):
        from lodestar_amd.native import GpuContext

        self.ctx = GpuContext(0)
        self.keys = table_keys(golden)
        codes = self.ctx.load_pubkeys(b"".join(self.keys), 48)
        assert list(codes) == [0] * len(self.keys)
        self.ctx.set_committee_group(G_SIZES, SIZE_COMMITTEES)
        self.ctx.set_committee_group(G_STRUCT, STRUCT)

    def sign_lists(self, lists, msgs) -> list[bytes]:
        sks = [sum(table_sk(i) for i in lst) % O.R for lst in lists]
        out = self.ctx.sign(b"".join(s.to_bytes(32, "big") for s in sks), b"".join(msgs))
        return [s.tobytes() for s in out]

    def expected(self, lst) -> bytes:
        return ge.expected_aggregate(self.keys, lst)
