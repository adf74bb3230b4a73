"""CPU-only construction of the group-law edge inputs of tests/test_gpu_group_edges.py
(proved by tests/test_groupedge_cpu.py against the oracle): points of small prime order on
E1 and E2 outside G1 / G2, the walk of the |x| double-and-add chain that says which
additions such a point makes exceptional, negated keys and signatures, and the index-list
layouts that steer equal and opposite partial sums into chosen lanes and tree levels of the
wavefront pubkey aggregation (kernels/k_pk.hip k_pk_agg).

Nothing here touches the GPU library."""
from __future__ import annotations

import functools
import hashlib
import random

from oracle import bls_oracle as O

# cofactors of E1(Fp) and E2(Fp2): #E1 = H1 * r, #E2 = H2 * r  (H1 = 3 * 11^2 * ...,
# H2 = 13^2 * 23^2 * ...).  Never trusted: test_groupedge_cpu.py proves [N]pt = O.
H1 = 0x396C8C005555E1568C00AAAB0000AAAB
H2 = 0x5D543A95414E7F1091D50792876A202CD91DE4547085ABAA68A205B2E5A7DDFA628F1CB4D9E82EF21537E293A6691AE1616EC6E786F0C70CF1C38E31C7238E5
N1 = H1 * O.R
N2 = H2 * O.R

INF_PK48 = bytes([0xC0]) + bytes(47)
INF_PK96 = bytes([0x40]) + bytes(95)
INF_SIG96 = bytes([0xC0]) + bytes(95)

LANES = 64      # BLS_BLOCK: lanes of k_pk_agg's wavefront
AGG_MIN = 16    # BLS_AGG_WAVE_MIN: fewer keys take the serial stage_pk loop


def _h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


# ---------------------------------------------------------------------------
# points of small prime order
# ---------------------------------------------------------------------------
def e2_seed_points():
    """On-curve E2 points from 0x80 || 0...0 || x1 for x1 = 2, 3, ... (the search of
    tests/golden/make_golden.py, which stops at the first point off G2)."""
    x1 = 2
    while True:
        b = bytearray(96)
        b[0] = 0x80
        b[95] = x1
        code, pt = O.g2_decompress(bytes(b))
        if code == O.E_OK and pt is not None:
            yield x1, pt
        x1 += 1


def e1_seed_points():
    """On-curve E1 points (x, sqrt(x^3 + 4)) for x = 1, 2, ..."""
    x = 1
    while True:
        y = O.fp_sqrt((x ** 3 + 4) % O.P)
        if y is not None:
            yield x, (x, y)
        x += 1


def _low_order(curve, n_group: int, seeds, ell: int):
    """T = [N / ell^2] pt, or [ell] T when that still has order ell^2: a point of prime
    order ell from the first seed point with an ell-part (None never returned)."""
    assert n_group % (ell * ell) == 0 and n_group % (ell ** 3) != 0
    for tag, pt in seeds:
        t = curve.mul(pt, n_group // (ell * ell))
        if t is None:
            continue
        lt = curve.mul(t, ell)
        return tag, pt, (t if lt is None else lt)
    raise AssertionError("unreachable")


@functools.lru_cache(maxsize=None)
def low_order_e2(ell: int):
    """(x1 of the seed, the seed point, a point of order ell on E2) for ell in {13, 23}."""
    return _low_order(O.E2, N2, e2_seed_points(), ell)


@functools.lru_cache(maxsize=None)
def low_order_e1(ell: int):
    """(x of the seed, the seed point, a point of order 11 on E1)."""
    return _low_order(O.E1, N1, e1_seed_points(), ell)


ORDER3_E1 = ((0, 2), (0, O.P - 2))  # y^2 = 4 at x = 0: 2P = -P


@functools.lru_cache(maxsize=None)
def multiples_e2(ell: int, ks: tuple):
    """[k]T for the order-ell E2 point T, k in ks, as affine points."""
    t = low_order_e2(ell)[2]
    return tuple(O.E2.mul(t, k) for k in ks)


def q13_multiples():
    """all twelve non-zero multiples of the order-13 point (both signs of each)"""
    return multiples_e2(13, tuple(range(1, 13)))


def q23_multiples():
    """a few multiples of the order-23 point, both signs among them"""
    return multiples_e2(23, (1, 2, 5, 11, 12, 22))


@functools.lru_cache(maxsize=None)
def low_order_sigs():
    """(twelve compressed order-13 signatures, six compressed order-23 ones)"""
    return (tuple(O.g2_compress(p) for p in q13_multiples()), tuple(O.g2_compress(p) for p in q23_multiples()))


@functools.lru_cache(maxsize=None)
def low_order_keys():
    """E1 points of order 3 and 11 (both signs, a few multiples): [(name, point)]"""
    t = low_order_e1(11)[2]
    out = [("order3+", ORDER3_E1[0]), ("order3-", ORDER3_E1[1])]
    out += [("order11*%d" % k, O.E1.mul(t, k)) for k in (1, 2, 5, 10)]
    return tuple(out)


# ---------------------------------------------------------------------------
# which additions of the [|x|] chain a point of order ell makes exceptional
# ---------------------------------------------------------------------------
def prefix_walk(ell: int, k: int = O.X_ABS):
    """The left-to-right double-and-add of curve.hpp jac_mul_u64 (and of the cooperative
    pset_xchain programs) over the bits of k, for a base P of order ell: the accumulator
    before each step is [j]P for the bit prefix j.  Returns the exceptional steps as
    (bit index, kind):
      "dbl_inf"  doubling with j = 0 (mod ell): the accumulator is infinity
      "add_inf"  addition with j = 0: infinity + P
      "add_dbl"  addition with j = 1: P + P
      "add_neg"  addition with j = -1: (-P) + P = infinity
    An empty list means P stays on the ordinary branches of both formulas."""
    bits = bin(k)[3:]  # the top bit loads P
    j, out = 1, []
    for n, bit in enumerate(bits):
        i = len(bits) - 1 - n
        if j % ell == 0:
            out.append((i, "dbl_inf"))
        j = 2 * j
        if bit == "1":
            m = j % ell
            if m == 0:
                out.append((i, "add_inf"))
            elif m == 1:
                out.append((i, "add_dbl"))
            elif m == ell - 1:
                out.append((i, "add_neg"))
            j += 1
    assert j == k
    return out


# ---------------------------------------------------------------------------
# negation in the compressed encodings
# ---------------------------------------------------------------------------
def neg_compressed(b: bytes) -> bytes:
    """-P of a compressed G1 (48 B) or G2 (96 B) point that is not infinity: the sort
    bit 0x20 of byte 0 flipped (y != 0 on both curves for points of odd order)."""
    assert b[0] & 0x80 and not b[0] & 0x40
    return bytes([b[0] ^ 0x20]) + b[1:]


# ---------------------------------------------------------------------------
# pubkey table and index lists of the aggregation tests
# ---------------------------------------------------------------------------
N_BASE = 32          # interop keys 0..31 at indices 0..31
NEG_BASE = 32        # -key j at index 32 + j, j < 8
N_NEG = 8
INF_INDEX = 40       # the compressed infinity key


def table_keys(golden, with_infinity: bool = True) -> list[bytes]:
    """the 48-byte keys of the module's own table, in index order"""
    base = [bytes.fromhex(h) for h in golden["kat2_interop_pubkeys"][:N_BASE]]
    keys = base + [neg_compressed(k) for k in base[:N_NEG]]
    if with_infinity:
        keys.append(INF_PK48)
    return keys


@functools.lru_cache(maxsize=None)
def _table_points(keys: tuple):
    out = []
    for k in keys:
        code, pt = O.g1_decompress(k)
        assert code == O.E_OK
        out.append(pt)
    return tuple(out)


def expected_aggregate(keys, lst) -> bytes:
    """oracle.aggregate_pubkeys + g1_serialize of the listed table entries"""
    pts = _table_points(tuple(keys))
    return O.g1_serialize(O.aggregate_pubkeys([pts[i] for i in lst]))


def neg(j: int) -> int:
    assert j < N_NEG
    return NEG_BASE + j


EQUAL_SIZES = (2, 3, 15, 16, 17, 63, 64, 65, 128, 129, 200)


def pk_layouts(with_infinity: bool = True):
    """[(name, index list)]: every list of section 2 of the group-edge tests but the
    seeded random ones.  Lane l of k_pk_agg sums positions l, l + 64, ... of a list of >=
    16 keys; tree level s (32, 16, 8, 4, 2, 1) adds lane l + s into lane l < s."""
    L = []
    for n in EQUAL_SIZES:
        L.append(("all_equal_n%d" % n, [3] * n))
    L.append(("halves_opposite_level32", [2] * 32 + [neg(2)] * 32))
    L.append(("every_lane_cancels", [5] * 64 + [neg(5)] * 64))
    # cancel, then continue
    L.append(("small_a_nega_b", [1, neg(1), 9]))
    L.append(("small_a_b_nega", [1, 9, neg(1)]))
    fill = [8 + (i % 24) for i in range(80)]  # keys 8..31: no negation of them in the table
    same_lane = list(fill)
    same_lane[5], same_lane[5 + LANES] = 0, neg(0)
    L.append(("pair_in_one_lane", same_lane))
    sibling = fill[:64]
    sibling[5], sibling[5 + 32] = 0, neg(0)
    L.append(("pair_in_sibling_lanes", sibling))
    L.append(("64_cancel_pairwise_then_65th", [i % 8 for i in range(32)] + [neg(i % 8) for i in range(32)] + [17]))
    # later-level collisions
    L.append(("P16_negP16_Q32_dbl_levels_8_4_2_1", [4] * 16 + [neg(4)] * 16 + [11] * 32))
    L.append(("P16_negP16_cancel_level16", [6] * 16 + [neg(6)] * 16))
    L.append(("P16_P16_dbl_level16", [6] * 32))
    L.append(("P8_negP8_cancel_level8", [7] * 8 + [neg(7)] * 8))
    L.append(("even_odd_opposite_cancel_level1", [v for j in range(8) for v in (j, neg(j))]))
    # odd lanes hold the even lanes' keys in another order: equal points with different Z
    ev = list(range(8))
    od = [ev[(j + 4) % 8] for j in range(8)]
    L.append(("even_odd_equal_dbl_level1", [v for j in range(8) for v in (ev[j], od[j])]))
    if with_infinity:
        L.append(("inf_alone", [INF_INDEX]))
        L.append(("inf_first", [INF_INDEX, 3]))
        L.append(("inf_middle", [3, INF_INDEX, 5]))
        L.append(("inf_x16_whole_list", [INF_INDEX] * 16))
        wide = [8 + (i % 24) for i in range(70)]
        for pos in (0, 13, 63, 64, 69):
            wide[pos] = INF_INDEX
        L.append(("inf_inside_70", wide))
        L.append(("inf_lane_then_cancel", [INF_INDEX] * 32 + [2] * 16 + [neg(2)] * 16))
    return L


def random_pk_lists(seed: int = 20261019, count: int = 40):
    """seeded lists of 1..130 indices drawn with replacement from {0..7, 32..39}"""
    rng = random.Random(seed)
    pool = list(range(8)) + [neg(j) for j in range(8)]
    sizes = [1, 15, 16, 17, 64, 65, 130] + [rng.randrange(1, 131) for _ in range(count - 7)]
    return [[rng.choice(pool) for _ in range(n)] for n in sizes]


# ---------------------------------------------------------------------------
# low-order signatures inside a call of single-set batchable requests
# ---------------------------------------------------------------------------
LOW_CALL_N = 48                    # three chunks of 16 requests (worker.ts:17,56)
LOW_POS13 = (0, 7, 15, 20, 32)     # chunk 0's first / a middle / its last request, ...
LOW_POS23 = (26, 31, 45, 47)       # ... and every slot of a wavefront of 2 and of 3 sets


def expected_worker(reqs):
    """(verdicts, batch_retries, batch_sigs_success) of one worker message from the oracle's
    worker semantics (oracle.verify_many_signature_sets, worker.ts:32-108) over outcome
    tokens: reqs is [(batchable, [token, ...])], a token the set's known outcome (1 valid,
    0 invalid, -code).  The predicate is the one of tests/test_gpu_parity.py
    _expected_stats (maybeBatch.ts:16-39): every signature is decoded first and a decode
    error throws; one set alone verifies deterministically (an infinity signature throws
    ZERO_SIGNATURE there, and only makes a batch false); otherwise the batch is valid iff
    every set is."""
    zero = -O.E_ZERO_SIGNATURE

    def maybe_batch(tokens):
        if len(tokens) == 0:
            raise O.BlsError(O.E_EMPTY_SET)
        for t in tokens:
            if t < 0 and t != zero:
                raise O.BlsError(-t)
        if len(tokens) == 1 and tokens[0] == zero:
            raise O.BlsError(O.E_ZERO_SIGNATURE)
        return all(t == 1 for t in tokens)

    res, retries, ok = O.verify_many_signature_sets([(b, list(ts)) for b, ts in reqs], maybe_batch)
    return [(1 if r[1] else 0) if r[0] == "success" else -r[1].code for r in res], retries, ok


# ---------------------------------------------------------------------------
# secret keys behind the table (signing the aggregate sets)
# ---------------------------------------------------------------------------
def table_sk(i: int) -> int:
    """the scalar of table entry i: interop key, its negation, or 0 for infinity"""
    if i < N_BASE:
        return O.interop_secret_key(i)
    if i < NEG_BASE + N_NEG:
        return (-O.interop_secret_key(i - NEG_BASE)) % O.R
    assert i == INF_INDEX
    return 0


def list_sk(lst) -> int:
    return sum(table_sk(i) for i in lst) % O.R
