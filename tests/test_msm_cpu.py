"""The Pippenger signature sum without a GPU: the CPU restatement of its stages and of the
bucket blocks' tickets (tests/native/msm_host.cpp: the same bls/msm.hpp bodies the
kernels compile, a wavefront as a loop over its lanes, a launch as a loop over its
blocks), once plain and once under AddressSanitizer + UBSan as a stand-alone program."""
from __future__ import annotations

import subprocess

from lodestar_amd import _abi
from lodestar_amd.build import build_msm_host


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1].split()
    # 16 cases x 6 block orders, each checking the 1,026 state words at least
    assert last[0] == "ok" and int(last[1]) > 16 * 6 * 1026, out.stdout[-500:]


def test_msm_sum_and_block_orders():
    """n = 2, 63, 64, 65, 256 with sets not live, a bucket over several segments and a
    cancelling pair: the virtual set equals the left-to-right sum of [r_i] sig_i; with the
    16 bucket blocks forward, reversed and shuffled, one block per window runs the window
    body, the window sums and the final point are bit-identical, every ticket returns to 0"""
    _run(build_msm_host(verbose=False))


def test_msm_under_sanitizers(tmp_path):
    """the same stand-alone program compiled with -fsanitize=address,undefined: any report
    makes it exit non-zero"""
    exe = build_msm_host(verbose=False, out=tmp_path / "msm_host_san",
                         extra=["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _run(exe)


def test_serial_flag_is_the_next_free_debug_bit():
    flags = [v for k, v in vars(_abi).items() if k.startswith("DEBUG_") and isinstance(v, int)]
    assert _abi.DEBUG_MSM_SERIAL == 0x20000 and flags.count(_abi.DEBUG_MSM_SERIAL) == 1
    assert _abi.DEBUG_MSM_SERIAL & (0x300 | 0x7000) == 0  # clear of the PACK and MLF_PL fields
