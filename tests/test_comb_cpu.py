"""The pubkey table's fixed-base comb without a GPU: bls/curve.hpp g1_comb_build /
g1_comb_mul (what k_comb_build and k_chain's role 3 run per lane) compiled for the host
(tests/native/comb_host.cpp), against the GLV chain bit for bit and against the oracle's
[(a + b mu) mod r] P, mu = -x^2 mod r; once more under AddressSanitizer + UBSan as a
stand-alone program."""
from __future__ import annotations

import random
import subprocess

import pytest

from lodestar_amd.build import build_comb_host

EDGE = [(1, 0), (0, 1), (0xFFFFFFFF, 0xFFFFFFFF), (0x01010101, 0), (0, 0x80808080), (0x000000FF, 0xFF000000)]
N_KEYS = 32


def _self_check(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 900, out.stdout[-500:]
    return lines


def test_comb_equals_glv_chain_and_rows_equal_multiples():
    """32 keys [k] g1 x (6 edge + 8 random scalars): comb == jac_mul_glv in affine form, bit
    for bit; each of the 15 rows == [sum bit_t(k) 2^(8t)] P; the infinity key reports no
    comb.  On-curve keys outside G1 (first small x with x^3 + 4 a square, not
    cofactor-cleared): observed -- x = 0 gives (0, 2), of order 3, and the builder reports no
    comb (an entry is infinity); the first x >= 1 builds, and its rows give jac_mul_glv's
    element for every scalar.  The program fails unless it sees exactly that."""
    lines = _self_check(build_comb_host(verbose=False))
    assert "outside_g1 refused=1 equal=1" in lines


def test_comb_under_sanitizers(tmp_path):
    """the same stand-alone program compiled with -fsanitize=address,undefined: any report
    makes it exit non-zero"""
    exe = build_comb_host(verbose=False, out=tmp_path / "comb_host_san",
                          extra=["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _self_check(exe)


@pytest.fixture(scope="module")
def records(golden, oracle, tmp_path_factory):
    """(cases, output lines): the 32 first interop keys, each with one random (a, b) and the
    six edge scalars; the infinity key; the first on-curve x >= 0 points outside G1."""
    rng = random.Random(0xC0B)
    keys = []
    for h in golden["kat2_interop_pubkeys"][:N_KEYS]:
        code, pt = oracle.g1_decompress(bytes.fromhex(h))
        assert code == 0
        keys.append(pt)
    cases = [(pt, a, b) for pt in keys for a, b in [(rng.getrandbits(32), rng.getrandbits(32))] + EDGE]
    cases.append((None, 5, 7))
    outside = []
    x = 0
    while len(outside) < 2:
        y = oracle.fp_sqrt((x ** 3 + 4) % oracle.P)
        if y is not None:
            outside.append((x, y))
        x += 1
    cases += [(pt, a, b) for pt in outside for a, b in [(rng.getrandbits(32), rng.getrandbits(32)), EDGE[2]]]
    path = tmp_path_factory.mktemp("comb") / "records.bin"
    path.write_bytes(b"".join(oracle.g1_serialize(pt) + a.to_bytes(4, "little") + b.to_bytes(4, "little")
                              for pt, a, b in cases))
    out = subprocess.run([str(build_comb_host(verbose=False)), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert len(lines) == len(cases)
    return cases, lines, len(keys) * (1 + len(EDGE))


def test_comb_matches_oracle_scalar_multiple(records, oracle):
    """comb == GLV == the oracle's [(a + b mu) mod r] P for 32 interop keys x (one random
    scalar + the six edge scalars)"""
    cases, lines, n_g1 = records
    mu = (-oracle.X_ABS * oracle.X_ABS) % oracle.R
    for (pt, a, b), (status, built, comb, glv, _rows) in zip(cases[:n_g1], lines[:n_g1]):
        assert (status, built) == ("0", "1")
        want = oracle.g1_serialize(oracle.E1.mul(pt, (a + b * mu) % oracle.R)).hex()
        assert comb == glv == want, (hex(a), hex(b))


def test_rows_match_oracle_multiples(records, oracle):
    """row k of every key == [sum bit_t(k) 2^(8t)] P from the oracle"""
    cases, lines, n_g1 = records
    for (pt, _a, _b), ln in list(zip(cases[:n_g1], lines[:n_g1]))[::1 + len(EDGE)]:
        rows = ln[4]
        assert len(rows) == 15 * 192
        for k in range(1, 16):
            e = sum(1 << (8 * t) for t in range(4) if (k >> t) & 1)
            assert rows[192 * (k - 1): 192 * k] == oracle.g1_serialize(oracle.E1.mul(pt, e)).hex(), k


def test_infinity_and_keys_outside_g1(records, oracle):
    """the infinity key reports no comb.  Outside G1 the oracle's scalar multiple is no
    reference (mu is sigma's eigenvalue on G1 only): observed -- (0, 2), of order 3, reports
    no comb; the next point builds and equals the GLV chain's element ([a]P + [b]sigma(P)
    by the oracle's own curve arithmetic)."""
    cases, lines, n_g1 = records
    assert lines[n_g1][:2] == ["0", "0"] and lines[n_g1][2] == "-"
    beta = None
    for (pt, a, b), (status, built, comb, glv, _rows) in zip(cases[n_g1 + 1:], lines[n_g1 + 1:]):
        assert status == "0" and oracle.E1.on_curve(pt) and not oracle.g1_in_subgroup(pt)
        if pt[0] == 0:
            assert built == "0" and oracle.E1.mul(pt, 3) is None
            continue
        assert built == "1" and comb == glv
        if beta is None:  # the beta of sigma: the cube root of unity with sigma = [mu] on G1
            g = oracle.G1
            mu = (-oracle.X_ABS * oracle.X_ABS) % oracle.R
            beta = oracle.E1.mul(g, mu)[0] * pow(g[0], -1, oracle.P) % oracle.P
        sig = (pt[0] * beta % oracle.P, pt[1])
        want = oracle.E1.add(oracle.E1.mul(pt, a), oracle.E1.mul(sig, b))
        assert comb == oracle.g1_serialize(want).hex()
