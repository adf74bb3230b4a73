"""A/B of the committee-bitfield input form against index lists on one cfg3-shaped call
(profiles/committees_ab.json).

One non-batchable request of 129 aggregate sets over 512-member committees drawn without
replacement from an n-key table (workload seed 1), each with round(1 % of 512) = 5 absentees:
99 % participation.  The same sets go out in both forms, alternated in one process on one
context and one build, REPS calls each after WARMUP:
  lists       bls_gpu_verify on the expanded index lists (129 x 507 indices)
  committees  bls_gpu_verify_committees on (committee, bits) over a registered group
For each: stage_ms[1] (the pubkey stage: k_pk + k_pk_agg + k_pk_bits), the call's device_ms
and wall time, as median / min / max, and the bytes of the call's key-selection arrays
(pk_indices against set_committee + set_bits_off + bits) and of all its input arrays.  Also
the registration: wall time of bls_gpu_set_committee_group and the group's device bytes.

    python tools/committees_ab.py [--keys 1048576] [--reps 25] [--out profiles/committees_ab.json]
"""
from __future__ import annotations

import argparse
import json
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from lodestar_amd import workloads as W  # noqa: E402
from lodestar_amd.native import GpuContext, pack_requests  # noqa: E402

WARMUP = 3
N_SETS, MEMBERS, ABSENT = 129, 512, 5
GROUP = 0


def summary(xs: list[float]) -> dict:
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def input_bytes(pb) -> dict:
    arrays = {f: getattr(pb, f) for f in ("req_set_offsets", "req_batchable", "messages", "signatures", "set_pk_offsets",
                                          "pk_indices", "set_committee", "set_bits_off", "bits")}
    sizes = {f: int(a.nbytes) for f, a in arrays.items() if a is not None}
    select = [f for f in ("pk_indices", "set_committee", "set_bits_off", "bits") if f in sizes]
    return {"key_selection": sum(sizes[f] for f in select), "all_inputs": sum(sizes.values()), "arrays": sizes}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "committees_ab.json"))
    a = ap.parse_args()

    rng = random.Random(1)
    with GpuContext(0) as ctx:
        t0 = time.perf_counter()
        W.load_table([ctx], a.keys)
        table_s = time.perf_counter() - t0
        sks = W.interop_sks(a.keys)
        committees = [rng.sample(range(a.keys), MEMBERS) for _ in range(N_SETS)]
        absent = [set(rng.sample(range(MEMBERS), ABSENT)) for _ in range(N_SETS)]
        t0 = time.perf_counter()
        ctx.set_committee_group(GROUP, committees)
        register_ms = (time.perf_counter() - t0) * 1e3
        info = ctx.committee_group_info(GROUP)

        lists, fields = [], []
        for members, gone in zip(committees, absent):
            bits = bytearray(MEMBERS // 8)
            for j in range(MEMBERS):
                if j not in gone:
                    bits[j >> 3] |= 1 << (j & 7)
            fields.append(bytes(bits))
            lists.append([m for j, m in enumerate(members) if j not in gone])
        msgs = [W.message(j, b"CMTE") for j in range(N_SETS)]
        sigs = W._sign_all(ctx, [sum(sks[i] for i in lst) % W.R_ORDER for lst in lists], msgs)
        seed = (1).to_bytes(32, "big")
        pb = {
            "lists": pack_requests([(False, [(lst, m, s) for lst, m, s in zip(lists, msgs, sigs)])], seed=seed),
            "committees": pack_requests([(False, [{"committee": (GROUP, k), "bits": f, "message": m, "signature": s}
                                                  for k, (f, m, s) in enumerate(zip(fields, msgs, sigs))])], seed=seed),
        }
        run = {"lists": ctx.verify_packed, "committees": ctx.verify_committees_packed}
        rec = {k: {"pk_stage_ms": [], "device_ms": [], "wall_ms": []} for k in pb}
        for it in range(WARMUP + a.reps):
            for form in ("lists", "committees"):
                t0 = time.perf_counter()
                v, st = run[form](pb[form])
                wall = (time.perf_counter() - t0) * 1e3
                assert list(v) == [1], (form, list(v))
                if it >= WARMUP:
                    rec[form]["pk_stage_ms"].append(st.stage_ms[1])
                    rec[form]["device_ms"].append(st.device_ms)
                    rec[form]["wall_ms"].append(wall)
        out = {
            "shape": {"sets": N_SETS, "members": MEMBERS, "absent_per_set": ABSENT, "table_keys": a.keys,
                      "workload_seed": 1, "reps": a.reps, "warmup": WARMUP, "request": "one non-batchable request"},
            "table_build_s": round(table_s, 2),
            "registration": {"wall_ms": round(register_ms, 3), **info},
        }
        for form in pb:
            out[form] = {k: summary(v) for k, v in rec[form].items()}
            out[form]["h2d_bytes"] = input_bytes(pb[form])
        out["pk_stage_speedup"] = round(out["lists"]["pk_stage_ms"]["median"] / out["committees"]["pk_stage_ms"]["median"], 3)
        out["wall_p50_ratio"] = round(out["lists"]["wall_ms"]["median"] / out["committees"]["wall_ms"]["median"], 4)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
