"""Reference interpreter of an emitted cooperative-program table (tools/gen_coop.py emit;
lodestar_amd/_native/coop_tables.bin.gz is what the library loads): coop.hpp coop_step's
semantics lane by lane, as exact arithmetic mod p on plain (non-Montgomery) residues.

The table is parsed once (CoopTable); a program's steps are decoded on first use."""
from __future__ import annotations

import gzip
import struct
from pathlib import Path

from tests._codec import P

R_INV = pow(1 << 384, -1, P)
_OP = struct.Struct("<HBBBBBB8H8H8h8h8x")  # coop.hpp CoopOp, 80 bytes


class CoopTable:
    def __init__(self, raw: bytes):
        self.raw = raw
        magic, self.version, nc, nprog, self.n_steps = struct.unpack_from("<4sIIII", raw, 0)
        assert magic == b"BLSC"
        off = 20
        consts = [int.from_bytes(raw[off + 48 * k: off + 48 * (k + 1)], "little") for k in range(nc)]
        self.consts = [c * R_INV % P for c in consts]  # the bank is in Montgomery form
        off += 48 * nc
        self.programs = {}  # name -> (first, n_steps, n_slots, n_mul), in table order
        for _ in range(nprog):
            nm = raw[off: off + 32].rstrip(b"\0").decode()
            self.programs[nm] = struct.unpack_from("<IIII", raw, off + 32)
            off += 48
        self.ops_off = off
        assert off + 80 * 64 * self.n_steps == len(raw)
        self._steps = {}

    @classmethod
    def from_file(cls, path) -> "CoopTable":
        path = Path(path)
        return cls(gzip.decompress(path.read_bytes()) if path.suffix == ".gz" else path.read_bytes())

    def n_slots(self, name: str) -> int:
        return self.programs[name][2]

    def steps(self, name: str):
        """[(gp, gl, lanes)] per step: the product / combination lane-group sizes and the
        lanes' (out, kind, na, nb, a[8], b[8], ca[8], cb[8]); the per-step fields (largest
        term counts, flags) are checked to be what every lane says."""
        if name in self._steps:
            return self._steps[name]
        first, n, _, _ = self.programs[name]
        L = 128 if name.endswith("_w2") else 64  # two-wavefront programs: steps of 128 ops
        out = []
        for s in range(n):
            rec = first + s * (L // 64)
            lanes = [_OP.unpack_from(self.raw, self.ops_off + 80 * (64 * rec + ln)) for ln in range(L)]
            ma, mb, fl = lanes[0][4:7]
            assert all(x[4:7] == (ma, mb, fl) for x in lanes)
            assert ma == max((x[2] for x in lanes if x[1]), default=0)
            assert mb == max((x[3] for x in lanes if x[1] == 1), default=0)
            gp, gl = 1 << ((fl >> 2) & 3), 1 << ((fl >> 4) & 3)
            out.append((gp, gl, [(x[0], x[1], x[2], x[3], x[7:15], x[15:23], x[23:31], x[31:39]) for x in lanes]))
        self._steps[name] = out
        return out

    def run(self, name: str, frame: list) -> int:
        """Run program `name` on `frame` (plain residues, updated in place); returns the
        zero-check flag word.  Kinds 1 (product), 2 (combination, or its part in a lane
        group of the step's combination group size gl), 3 / 4 (part of a product's operand
        a / b in a lane group of size gp: each half of the group sums one operand, every
        lane multiplies); the group's first lane writes."""
        n_slots = self.n_slots(name)
        cvals = self.consts
        flag = 0
        for gp, gl, lanes in self.steps(name):

            def lin(refs, cfs, k):
                return sum(cf * (frame[r] if r < n_slots else cvals[r - n_slots]) for r, cf in zip(refs[:k], cfs[:k])) % P

            vals = []
            for out, kind, na, nb, ra, rb, ca, cb in lanes:
                v = lin(ra, ca, na) if kind else 0
                if kind == 1:
                    v = v * lin(rb, cb, nb) % P
                vals.append(v)
            res = list(vals)
            for ln, (out, kind, *_r) in enumerate(lanes):
                if kind == 2 and gl > 1:
                    base = ln & ~(gl - 1)
                    assert all(lanes[base + k][1] == 2 for k in range(gl) if lanes[base + k][1])
                    res[ln] = sum(vals[base: base + gl]) % P
                elif kind in (3, 4):
                    base, h = ln & ~(gp - 1), gp // 2
                    assert [lanes[base + k][1] for k in range(gp)] == [3] * h + [4] * h
                    res[ln] = sum(vals[base: base + h]) * sum(vals[base + h: base + gp]) % P
            for ln, (out, kind, *_r) in enumerate(lanes):
                if kind == 0 or out == 0xFFFE:
                    continue
                if out >= 0xFFF0:
                    if res[ln] == 0:
                        flag |= 1 if out == 0xFFFF else 1 << (out - 0xFFF0)
                else:
                    frame[out] = res[ln]
        return flag

    def accumulators(self, name: str):
        """Every 13-limb accumulator acc_reduce sees while program `name` runs, as the list
        of its coefficients: one lane's operand, or the operands the DPP butterflies add
        together (the gl lanes of a combination group; each half of a product group)."""
        for gp, gl, lanes in self.steps(name):
            for ln, (out, kind, na, nb, ra, rb, ca, cb) in enumerate(lanes):
                if kind == 1:
                    yield list(ca[:na])
                    yield list(cb[:nb])
                elif kind == 2 and gl > 1:
                    base = ln & ~(gl - 1)
                    if ln == base:
                        yield [c for k in range(gl) if lanes[base + k][1] for c in lanes[base + k][6][:lanes[base + k][2]]]
                elif kind == 2:
                    yield list(ca[:na])
                elif kind in (3, 4):
                    base, h = ln & ~(gp - 1), gp // 2
                    if ln == base or ln == base + h:
                        yield [c for k in range(h) for c in lanes[ln + k][6][:lanes[ln + k][2]]]
