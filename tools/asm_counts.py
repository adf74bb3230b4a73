#!/usr/bin/env python3
"""Static instruction counts per function of a gfx950 assembly listing, the table of
DESIGN.md §7i / profiles/ab_fp2_prim.json:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include -I lodestar_amd/csrc -S \\
        --cuda-device-only lodestar_amd/csrc/kernels/k_mlq.hip -o k_mlq.s
    python tools/asm_counts.py k_mlq.s [name substring ...]

Every instruction counts as one issue slot (s_nop included).  Per function: the total,
multiply-adds, no-ops, pure moves (v_mov, v_accvgpr_*), add / sub / select glue, scratch
loads and stores, LDS operations, calls, and the VGPRs and scratch bytes the listing states.
"""
import collections
import re
import sys


def functions(text: str) -> dict:
    out = {}
    for f in re.split(r"\n(?=_Z\w+:)", text):
        m = re.match(r"(_Z\w+):", f)
        if not m:
            continue
        body = f.split(".Lfunc_end")[0]
        ins = [ln.strip().split()[0] for ln in body.splitlines()
               if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
        c = collections.Counter(ins)

        def g(*prefixes):
            return sum(v for k, v in c.items() if k.startswith(prefixes))

        nv = re.search(r"; NumVgprs: (\d+)", f)
        sc = re.search(r"; ScratchSize: (\d+)", f)
        out[m.group(1)] = {
            "issue_slots": len(ins), "mads": g("v_mad_u64", "v_mad_i64"), "s_nop": g("s_nop"),
            "moves": g("v_mov", "v_accvgpr"),
            "add_sub_select": g("v_addc", "v_subb", "v_and_b32", "v_cndmask", "v_add_co", "v_sub_co"),
            "scratch_loads": g("scratch_load"), "scratch_stores": g("scratch_store"), "lds_ops": g("ds_"),
            "calls": g("s_swappc"), "vgprs": int(nv.group(1)) if nv else None,
            "scratch_bytes": int(sc.group(1)) if sc else None}
    return out


if __name__ == "__main__":
    want = sys.argv[2:]
    for name, d in functions(open(sys.argv[1]).read()).items():
        if not want or any(w in name for w in want):
            print(name, " ".join(f"{k}={v}" for k, v in d.items()))
