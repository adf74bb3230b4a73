"""A/B of bls_gpu_verify_deposits against what a host could do before it
(profiles/deposits_ab.json).

For n valid deposits, alternated in one process, REPS repetitions after WARMUP:
  old    validate_pubkeys + ssz_roots + load_pubkeys into a scratch context + verify_packed
         of n one-set batchable requests over the loaded indices.  Only the verify call
         reports device time (stats.device_ms); the three helper calls copy in, run one
         kernel, copy out and synchronise, so each is timed by a host clock around the call.
         old_ms = their three wall times + the verify call's device_ms; old_wall_ms = the
         four wall times.
  new    one verify_deposits_packed: device_ms, its wall time, stage_ms (stage 1 is the front
         kernel k_deposit alone)
  fused  the same with $BLS_DEPOSIT_FUSED=1: one lane per deposit doing key and root
Medians, and min / max as the run-to-run spread.

    python tools/deposits_ab.py [--sizes 16,1024,16384] [--reps 20] [--out profiles/deposits_ab.json]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from lodestar_amd._abi import SSZ_DEPOSIT_MESSAGE  # noqa: E402
from lodestar_amd.deposits import deposit_domain  # noqa: E402
from lodestar_amd.native import GpuContext, PackedBatch, PackedDeposits  # noqa: E402

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
WARMUP = 2


def fixture(ctx: GpuContext, n: int, domain: bytes):
    """n valid deposits as arrays: keys, withdrawal credentials, amounts, signatures, roots"""
    sks = b"".join((int.from_bytes(hashlib.sha256(b"ab sk%d" % i).digest(), "little") % R_ORDER).to_bytes(32, "big")
                   for i in range(n))
    pks = ctx.sk_to_pk(sks)
    wcs = np.frombuffer(b"".join(hashlib.sha256(b"ab wc%d" % i).digest() for i in range(n)), np.uint8).reshape(n, 32)
    amts = np.frombuffer(b"".join((32 * 10**9 + i).to_bytes(8, "little") for i in range(n)), np.uint8).reshape(n, 8)
    objs = np.ascontiguousarray(np.concatenate([pks, wcs, amts], axis=1))
    roots = ctx.ssz_roots(SSZ_DEPOSIT_MESSAGE, objs, domain)
    sigs = ctx.sign(sks, roots)
    return pks, wcs, amts, objs, sigs


def summary(xs: list[float]) -> dict:
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def wall_ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def measure(n: int, reps: int, domain: bytes) -> dict:
    ctx, scratch = GpuContext(0), GpuContext(0)
    try:
        pks, wcs, amts, objs, sigs = fixture(ctx, n, domain)
        seed = bytes(range(32))
        pd = PackedDeposits(pubkeys48=pks.reshape(-1), withdrawal_credentials=wcs.reshape(-1).copy(),
                            amounts=amts.reshape(-1).copy(), signatures=sigs.reshape(-1),
                            domain=np.frombuffer(domain, np.uint8).copy(), n=n, seed=seed)
        offs = np.arange(n + 1, dtype=np.uint32)
        rows = {k: [] for k in ("old_ms", "old_wall_ms", "old_validate", "old_roots", "old_load", "old_verify_dev",
                                "new_ms", "new_wall_ms", "new_front", "fused_ms", "fused_front")}
        new_stage, old_stage = [], []
        loaded = 0
        for rep in range(WARMUP + reps):
            # old: the four calls a host had to make
            codes, t_val = wall_ms(lambda: scratch.validate_pubkeys(pks, 48))
            roots, t_root = wall_ms(lambda: scratch.ssz_roots(SSZ_DEPOSIT_MESSAGE, objs, domain))
            lc, t_load = wall_ms(lambda: scratch.load_pubkeys(pks, 48))
            assert not codes.any() and not lc.any()
            pb = PackedBatch(req_set_offsets=offs, req_batchable=np.ones(n, np.uint8), messages=roots.reshape(-1),
                             signatures=sigs.reshape(-1), set_pk_offsets=offs,
                             pk_indices=np.arange(loaded, loaded + n, dtype=np.uint32), seed=seed)
            loaded += n
            (v_old, st_old), t_ver = wall_ms(lambda: scratch.verify_packed(pb))
            # new, in both front-kernel shapes
            os.environ.pop("BLS_DEPOSIT_FUSED", None)
            (rc, v_new, st_new), t_new = wall_ms(lambda: ctx.verify_deposits_packed(pd))
            os.environ["BLS_DEPOSIT_FUSED"] = "1"
            rc_f, v_f, st_f = ctx.verify_deposits_packed(pd)
            os.environ.pop("BLS_DEPOSIT_FUSED", None)
            assert rc == 0 and rc_f == 0 and (v_old == 1).all() and (v_new == 1).all() and (v_f == 1).all()
            if rep < WARMUP:
                continue
            rows["old_validate"].append(t_val)
            rows["old_roots"].append(t_root)
            rows["old_load"].append(t_load)
            rows["old_verify_dev"].append(st_old.device_ms)
            rows["old_ms"].append(t_val + t_root + t_load + st_old.device_ms)
            rows["old_wall_ms"].append(t_val + t_root + t_load + t_ver)
            rows["new_ms"].append(st_new.device_ms)
            rows["new_wall_ms"].append(t_new)
            rows["new_front"].append(st_new.stage_ms[1])
            rows["fused_ms"].append(st_f.device_ms)
            rows["fused_front"].append(st_f.stage_ms[1])
            new_stage.append(list(st_new.stage_ms))
            old_stage.append(list(st_old.stage_ms))
        out = {"n": n, "reps": reps, **{k: summary(v) for k, v in rows.items()}}
        out["new_stage_ms_median"] = [round(statistics.median(c), 4) for c in zip(*new_stage)]
        out["old_verify_stage_ms_median"] = [round(statistics.median(c), 4) for c in zip(*old_stage)]
        out["new_stats"] = {f: getattr(st_new, f) for f in ("n_chunks", "merged_check", "pass_shape", "n_unique_msgs")}
        return out
    finally:
        ctx.close()
        scratch.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,1024,16384")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "deposits_ab.json"))
    a = ap.parse_args()
    domain = deposit_domain(bytes.fromhex("00000001"))
    res = {"tool": "tools/deposits_ab.py", "device": "MI355X (gfx950), one context per path",
           "note": "ms; old_ms = wall(validate_pubkeys) + wall(ssz_roots) + wall(load_pubkeys) + device_ms(verify); "
                   "new_ms = device_ms of bls_gpu_verify_deposits; *_front = stage_ms[1], the front kernel alone "
                   "(new: role-split k_deposit, fused: one lane per deposit); min / max = run-to-run spread",
           "sizes": [measure(int(s), a.reps, domain) for s in a.sizes.split(",")]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": a.out,
                      "sizes": [(s["n"], s["old_ms"]["median"], s["new_ms"]["median"]) for s in res["sizes"]]}))


if __name__ == "__main__":
    main()
