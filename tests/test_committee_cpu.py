"""Committee groups without a GPU: bls/committee.hpp (what bls_gpu_set_committee_group,
bls_gpu_verify_committees and k_pk_bits share) compiled for the host over a counting
allocator (tests/native/committee_host.cpp).  The program checks a registration's argument
validation case by case (each message names its committee), the slots' accounting over set /
replace / failed set / drop / close with no leak and no double free, committee_use_complement
at its tie (n = 8: c = 4 direct, c = 5 complement; n = 1; c = 0; c = n), the length and
padding checks for n = 1, 7, 8, 9, 64, 65, and the single-lane statement of the kernel's sum
over integers standing in for points, which must equal the plain sum over the set bits on
both branches.  Once plain and once under AddressSanitizer + UBSan, each as a stand-alone
program."""
from __future__ import annotations

import subprocess

from lodestar_amd.build import build_committee_host


def _self_check(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 3000, out.stdout[-500:]


def test_committee_bookkeeping_and_rules():
    _self_check(build_committee_host(verbose=False))


def test_under_address_sanitizer(tmp_path):
    """the same program with -fsanitize=address,undefined: any report makes it exit non-zero"""
    exe = build_committee_host(verbose=False, out=tmp_path / "committee_host_asan",
                               extra=["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                      "-fno-omit-frame-pointer"])
    _self_check(exe)
