"""A/B of the span input form against index lists on a block's Electra attestations
(profiles/spans_ab.json).

8 aggregate sets, each over 64 committees of 512 members (one slot's committees: 32,768 keys a
set), the committees disjoint slices of one shuffling of an n-key table (workload seed 1), each
with round(1 % of 512) = 5 absentees: 99 % participation.  The same sets go out in both forms,
alternated in one process on one context and one build, REPS calls each after WARMUP:
  lists   bls_gpu_aggregate_pubkeys on the expanded index lists (8 x 64 x 507 indices)
  spans   bls_gpu_aggregate_spans on (64 committee references, one 4096-byte field) a set
Both calls are synchronous (they end in a stream synchronise), so a pair of HIP events recorded
around one on an otherwise idle device spans its copies in, its kernels and its copies out; the
host's clock around the same call is recorded beside it.  The arrays are packed once, outside
the timed window, and the library is called directly.  The aggregate bytes and codes of the two
forms must be equal.  Also the registration: wall time of bls_gpu_set_committee_group for the 512
committees and the group's device bytes.

    python tools/spans_ab.py [--keys 1048576] [--reps 200] [--out profiles/spans_ab.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import random
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from lodestar_amd import workloads as W  # noqa: E402
from lodestar_amd._abi import COMMITTEE_REF  # noqa: E402
from lodestar_amd.native import GpuContext  # noqa: E402

WARMUP = 10
N_SETS, SEGMENTS, MEMBERS, ABSENT = 8, 64, 512, 5
GROUP = 0


def summary(xs: list[float]) -> dict:
    q = statistics.quantiles(xs, n=10)
    return {"median": round(statistics.median(xs), 4), "p10": round(q[0], 4), "p90": round(q[-1], 4),
            "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main() -> None:
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spans_ab.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    assert a.keys >= N_SETS * SEGMENTS * MEMBERS

    rng = random.Random(1)
    with GpuContext(0) as ctx:
        W.load_table([ctx], a.keys)
        shuffling = rng.sample(range(a.keys), N_SETS * SEGMENTS * MEMBERS)
        committees = [shuffling[k * MEMBERS:(k + 1) * MEMBERS] for k in range(N_SETS * SEGMENTS)]
        t0 = time.perf_counter()
        ctx.set_committee_group(GROUP, committees)
        register_ms = (time.perf_counter() - t0) * 1e3
        info = ctx.committee_group_info(GROUP)

        lists, fields = [], []
        for s in range(N_SETS):
            bits = bytearray(SEGMENTS * MEMBERS // 8)
            lst = []
            for k in range(SEGMENTS):
                gone = set(rng.sample(range(MEMBERS), ABSENT))
                for j, m in enumerate(committees[s * SEGMENTS + k]):
                    if j not in gone:
                        at = k * MEMBERS + j
                        bits[at >> 3] |= 1 << (at & 7)
                        lst.append(m)
            fields.append(bytes(bits))
            lists.append(lst)

        u32 = lambda xs: np.ascontiguousarray(xs, dtype=np.uint32)  # noqa: E731
        pk_off = u32(np.cumsum([0] + [len(lst) for lst in lists]))
        pk_idx = u32([m for lst in lists for m in lst])
        span_off = u32([SEGMENTS * s for s in range(N_SETS + 1)])
        span_refs = u32([COMMITTEE_REF(GROUP, k) for k in range(N_SETS * SEGMENTS)])
        bits_off = u32(np.cumsum([0] + [len(f) for f in fields]))
        bits = np.frombuffer(b"".join(fields), dtype=np.uint8).copy()
        ss, _keep = ctx._span_struct(span_off, span_refs, bits_off, bits)
        out = {f: np.zeros(96 * N_SETS, np.uint8) for f in ("lists", "spans")}
        codes = {f: np.full(N_SETS, -1, np.int32) for f in ("lists", "spans")}
        lib, h = ctx.lib, ctx._h

        def call_lists():
            return lib.bls_gpu_aggregate_pubkeys(h, pk_off.ctypes.data, pk_idx.ctypes.data, N_SETS,
                                                 out["lists"].ctypes.data, codes["lists"].ctypes.data)

        def call_spans():
            return lib.bls_gpu_aggregate_spans(h, ctypes.byref(ss), N_SETS, out["spans"].ctypes.data,
                                               codes["spans"].ctypes.data)

        run = {"lists": call_lists, "spans": call_spans}
        rec = {f: {"event_ms": [], "wall_ms": []} for f in run}
        for it in range(WARMUP + a.reps):
            for form in ("lists", "spans"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                rc = run[form]()
                wall = (time.perf_counter() - t0) * 1e3
                e1.record()
                e1.synchronize()
                assert rc == 0, (form, rc)
                if it >= WARMUP:
                    rec[form]["event_ms"].append(e0.elapsed_time(e1))
                    rec[form]["wall_ms"].append(wall)
        assert list(codes["lists"]) == list(codes["spans"]) == [0] * N_SETS
        assert out["lists"].tobytes() == out["spans"].tobytes(), "the two forms must give the same keys"

        res = {
            "shape": {"sets": N_SETS, "segments_per_set": SEGMENTS, "members_per_committee": MEMBERS,
                      "absent_per_committee": ABSENT, "keys_summed_per_set": len(lists[0]), "table_keys": a.keys,
                      "workload_seed": 1, "reps": a.reps, "warmup": WARMUP, "alternated": True},
            "registration": {"wall_ms": round(register_ms, 3), **info},
            "same_bytes_and_codes": True,
            "lists": {k: summary(v) for k, v in rec["lists"].items()},
            "spans": {k: summary(v) for k, v in rec["spans"].items()},
        }
        res["lists"]["h2d_bytes"] = int(pk_off.nbytes + pk_idx.nbytes)
        res["spans"]["h2d_bytes"] = int(span_off.nbytes + span_refs.nbytes + bits_off.nbytes + bits.nbytes)
        res["lists"]["point_additions_per_set"] = len(lists[0]) - 1
        res["spans"]["point_additions_per_set"] = SEGMENTS * (ABSENT + 1)
        res["event_speedup"] = round(res["lists"]["event_ms"]["median"] / res["spans"]["event_ms"]["median"], 3)
        res["wall_speedup"] = round(res["lists"]["wall_ms"]["median"] / res["spans"]["wall_ms"]["median"], 3)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
