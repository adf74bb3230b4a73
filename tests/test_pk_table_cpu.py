"""The shared key table's bookkeeping without a GPU: bls/pk_table.hpp (generations,
snapshots, appends; what bls_gpu_load_pubkeys and every verify entry point go through)
compiled for the host over an allocator that poisons freed buffers
(tests/native/pk_table_host.cpp).  Four reader threads take snapshots and check [0, n) of
the table and [0, comb_n) of the rows against the expected pattern while a loader appends
through several growths with one failing batch among them; further cases drop the rows
after a failed allocation and a failed build.  Once plain, once under ThreadSanitizer and
once under AddressSanitizer + UBSan, each as a stand-alone program."""
from __future__ import annotations

import subprocess

from lodestar_amd.build import build_pk_table_host


def _self_check(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100, out.stdout[-500:]


def test_snapshots_hold_under_appends():
    """readers never see a freed (poisoned) buffer or a slot at or above their n; a failing
    batch publishes nothing; sizes, capacities, device_bytes and the context count as the
    C ABI reports them; every buffer is freed exactly once and not written afterwards"""
    _self_check(build_pk_table_host(verbose=False))


def test_under_thread_sanitizer(tmp_path):
    """the same program with -fsanitize=thread: a data race between a loader and a reader,
    or between a free and a reader, makes it exit non-zero"""
    exe = build_pk_table_host(verbose=False, out=tmp_path / "pk_table_host_tsan",
                              extra=["-fsanitize=thread", "-fno-omit-frame-pointer", "-g"])
    _self_check(exe)


def test_under_address_sanitizer(tmp_path):
    """... and with -fsanitize=address,undefined"""
    exe = build_pk_table_host(verbose=False, out=tmp_path / "pk_table_host_asan",
                              extra=["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                     "-fno-omit-frame-pointer"])
    _self_check(exe)
