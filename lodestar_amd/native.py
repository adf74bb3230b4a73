"""Thin Python handle over the C-ABI (include/lodestar_bls.h) for one GPU.

`GpuContext` owns one `bls_gpu_ctx` (one device, one HIP stream, the device
pubkey table).  Buffers are numpy arrays handed over as raw pointers; the
library copies them into pinned staging, so nothing is retained after a call.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field

import numpy as np

from ._abi import (COMMITTEE_REF, ERR_ADMISSION, SET_NO_COMMITTEE, BlsAdmission, BlsBatch, BlsCommitteeInfo,
                   BlsCommitteeSets, BlsDepositBatch, BlsSameMsgBatch, BlsSpanSets, BlsStats, load_library)


def _ptr(a: np.ndarray | None):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def _u8(b) -> np.ndarray:
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


class NativeError(RuntimeError):
    pass


class AdmissionError(NativeError):
    """bls_gpu_init refused the context (BLS_ERR_ADMISSION): the HIP runtime's scratch for
    the process's contexts would pass the budget (include/lodestar_bls.h bls_admission)."""


def mapped_hip_runtime() -> list[str]:
    """Paths of the HIP runtime (libamdhip64) mapped into this process: /opt/rocm's when
    the library is loaded first, torch's bundled copy (same soname) when torch was
    imported before it -- the runtime the library's kernels then run under."""
    try:
        with open("/proc/self/maps") as f:
            return sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    except OSError:
        return []


class _DlInfo(ctypes.Structure):
    _fields_ = [("dli_fname", ctypes.c_char_p), ("dli_fbase", ctypes.c_void_p), ("dli_sname", ctypes.c_char_p),
                ("dli_saddr", ctypes.c_void_p)]


def library_hip_runtime() -> str | None:
    """The libamdhip64 file the library's HIP calls bind to: dlsym through the library's
    own handle searches its dependency scope, dladdr names the object that holds the
    symbol.  (/proc/self/maps may list two copies once torch is imported after the
    library: torch loads its bundled one by another name and never initialises it unless
    torch.cuda is used.)"""
    lib = load_library()
    try:
        addr = ctypes.cast(lib.hipGetDeviceCount, ctypes.c_void_p).value
    except AttributeError:
        return None
    info = _DlInfo()
    libc = ctypes.CDLL(None)
    libc.dladdr.argtypes = [ctypes.c_void_p, ctypes.POINTER(_DlInfo)]
    if not addr or libc.dladdr(ctypes.c_void_p(addr), ctypes.byref(info)) == 0 or not info.dli_fname:
        return None
    return os.path.realpath(info.dli_fname.decode())


def scratch_plan(n_normal: int, n_high: int, hw_queues: int = 0) -> tuple[bool, dict]:
    """The library's admission accounting for n_normal + n_high contexts (no device
    needed): (admissible, the bls_admission figures)."""
    a = BlsAdmission()
    rc = load_library().bls_scratch_plan(n_normal, n_high, hw_queues, ctypes.byref(a))
    return rc == 0, {f: getattr(a, f) for f, _ in BlsAdmission._fields_}


def admission(device: int = 0) -> dict:
    """The figures for the contexts open on `device` in this process."""
    a = BlsAdmission()
    load_library().bls_gpu_admission(device, ctypes.byref(a))
    return {f: getattr(a, f) for f, _ in BlsAdmission._fields_}


@dataclass
class PackedBatch:
    """SoA form of one verifyManySignatureSets call (bls_batch)."""

    req_set_offsets: np.ndarray  # uint32[n_reqs + 1]
    req_batchable: np.ndarray  # uint8[n_reqs]
    messages: np.ndarray  # uint8[n_sets * 32]
    signatures: np.ndarray  # uint8[n_sets * 96]
    pubkeys: np.ndarray | None = None  # uint8[n_sets * 96]
    set_pk_offsets: np.ndarray | None = None  # uint32[n_sets + 1]
    pk_indices: np.ndarray | None = None  # uint32[...]
    signature_lens: np.ndarray | None = None  # uint32[n_sets]
    seed: bytes | None = None
    # committee sets (bls_committee_sets; None: the batch has none and goes to bls_gpu_verify)
    set_committee: np.ndarray | None = None  # uint32[n_sets]: COMMITTEE_REF or SET_NO_COMMITTEE
    set_bits_off: np.ndarray | None = None  # uint32[n_sets + 1] byte offsets into bits
    bits: np.ndarray | None = None  # uint8[...]
    # span sets (bls_span_sets; None: the batch has none).  A batch holds committee sets or
    # span sets, never both: with a span in it, its committee sets are one-segment spans
    set_span_off: np.ndarray | None = None  # uint32[n_sets + 1] into span_refs
    span_refs: np.ndarray | None = None  # uint32[...]: COMMITTEE_REF per segment
    # the bls_batch view of these arrays, built on first use (GpuContext._batch_struct):
    # a pass of 64 calls re-packed its 64 structs under the GIL at every submission
    _cstruct: object = field(default=None, repr=False, compare=False)

    @property
    def n_sets(self) -> int:
        return int(self.req_set_offsets[-1])

    @property
    def n_reqs(self) -> int:
        return len(self.req_set_offsets) - 1


def pack_requests(requests, seed: bytes | None = None) -> PackedBatch:
    """requests: list of (batchable: bool, sets) where each set is (pk, msg32, sig).

    pk is either 96 raw bytes (uncompressed affine) or a list/tuple of device
    pubkey-table indices (all sets of one batch must use the same form).  sig may
    have any length (a length other than 96 yields BLST_INVALID_SIZE).

    A set may also be a dict {"committee": (group, index), "bits": bytes, "message": msg32,
    "signature": sig}: the aggregate of a registered committee's members at the set bits
    (GpuContext.set_committee_group).  Such sets mix with index-list sets, not with raw
    keys, and the batch then goes through GpuContext.verify_committees_packed.

    Or a dict {"committees": [(group, index), ...], "bits": bytes, "message": msg32,
    "signature": sig}: a span, the members of those committees concatenated in order under
    one field (an Electra attestation's committee_bits and aggregation_bits).  In a batch that
    holds any such dict a {"committee": ...} dict becomes a one-segment span, and the batch
    goes through GpuContext.verify_spans_packed."""
    offs = [0]
    batchable = []
    msgs, sigs, lens = [], [], []
    raw_pks, idx_offs, idx = [], [0], []
    table_mode = None
    refs, bits_offs, bits = [], [0], []
    span_offs, span_refs, any_span = [0], [], False
    for is_b, sets in requests:
        batchable.append(1 if is_b else 0)
        for one in sets:
            if isinstance(one, dict):
                pk, msg, sig = (), one["message"], one["signature"]
                if "committees" in one:
                    any_span = True
                    segs = [COMMITTEE_REF(int(g), int(i)) for g, i in one["committees"]]
                    if not segs:
                        raise ValueError("a span set names at least one committee")
                    span_refs.extend(segs)
                    refs.append(segs[0])  # (marks the set; a batch with a span ships span_refs, not refs)
                else:
                    group, index = one["committee"]
                    refs.append(COMMITTEE_REF(int(group), int(index)))
                    span_refs.append(refs[-1])
                bits.append(bytes(one["bits"]))
            else:
                pk, msg, sig = one
                refs.append(SET_NO_COMMITTEE)
                bits.append(b"")
            span_offs.append(len(span_refs))
            bits_offs.append(bits_offs[-1] + len(bits[-1]))
            this_table = not isinstance(pk, (bytes, bytearray, memoryview, np.ndarray))
            if table_mode is None:
                table_mode = this_table
            if table_mode != this_table:
                raise ValueError("mixed raw / table pubkeys in one batch")
            if table_mode:
                idx.extend(int(i) for i in pk)
                idx_offs.append(len(idx))
            else:
                pkb = bytes(pk)
                if len(pkb) != 96:
                    # the worker wire format is the 96-byte uncompressed key (index.ts:126,160);
                    # the C-ABI reads exactly 96 bytes per set
                    raise ValueError(f"raw pubkeys are 96 bytes (uncompressed affine), got {len(pkb)}")
                raw_pks.append(pkb)
            if len(msg) != 32:
                raise ValueError("signing roots are 32 bytes")
            msgs.append(bytes(msg))
            sb = bytes(sig)
            lens.append(len(sb))
            sigs.append(sb[:96].ljust(96, b"\0"))
        offs.append(len(msgs))
    n = len(msgs)
    pb = PackedBatch(
        req_set_offsets=np.array(offs, dtype=np.uint32),
        req_batchable=np.array(batchable, dtype=np.uint8),
        messages=np.frombuffer(b"".join(msgs), dtype=np.uint8).copy() if n else np.zeros(1, np.uint8),
        signatures=np.frombuffer(b"".join(sigs), dtype=np.uint8).copy() if n else np.zeros(1, np.uint8),
        seed=seed,
    )
    if any(L != 96 for L in lens):
        pb.signature_lens = np.array(lens, dtype=np.uint32)
    if table_mode:
        pb.set_pk_offsets = np.array(idx_offs, dtype=np.uint32)
        pb.pk_indices = np.array(idx if idx else [0], dtype=np.uint32)
        if any(r != SET_NO_COMMITTEE for r in refs):
            if any_span:
                pb.set_span_off = np.array(span_offs, dtype=np.uint32)
                pb.span_refs = np.array(span_refs, dtype=np.uint32)
            else:
                pb.set_committee = np.array(refs, dtype=np.uint32)
            pb.set_bits_off = np.array(bits_offs, dtype=np.uint32)
            pb.bits = np.frombuffer(b"".join(bits) or b"\0", dtype=np.uint8).copy()
    else:
        pb.pubkeys = np.frombuffer(b"".join(raw_pks), dtype=np.uint8).copy() if n else np.zeros(96, np.uint8)
    return pb


@dataclass
class PackedSameMsg:
    """SoA form of one bls_gpu_verify_same_message call (bls_same_msg_batch)."""

    job_set_offsets: np.ndarray  # uint32[n_jobs + 1]
    messages: np.ndarray  # uint8[n_jobs * 32]
    pk_indices: np.ndarray  # uint32[n_sets]
    signatures: np.ndarray  # uint8[n_sets * 96]
    seed: bytes | None = None

    @property
    def n_jobs(self) -> int:
        return len(self.job_set_offsets) - 1

    @property
    def n_sets(self) -> int:
        return int(self.job_set_offsets[-1])


def pack_same_message(jobs, seed: bytes | None = None) -> PackedSameMsg:
    """jobs: list of (message32, [table index...], [sig96...]), one signing root per job
    and one (index, signature) pair per set."""
    offs, msgs, idx, sigs = [0], [], [], []
    for msg, indices, job_sigs in jobs:
        if len(msg) != 32:
            raise ValueError("signing roots are 32 bytes")
        if len(indices) != len(job_sigs):
            raise ValueError("a same-message job carries one signature per key index")
        msgs.append(bytes(msg))
        idx.extend(int(i) for i in indices)
        for sig in job_sigs:
            sb = bytes(sig)
            if len(sb) != 96:
                raise ValueError("signatures are 96 bytes (compressed G2)")
            sigs.append(sb)
        offs.append(len(idx))
    return PackedSameMsg(
        job_set_offsets=np.array(offs, dtype=np.uint32),
        messages=np.frombuffer(b"".join(msgs), dtype=np.uint8).copy() if msgs else np.zeros(32, np.uint8),
        pk_indices=np.array(idx if idx else [0], dtype=np.uint32),
        signatures=np.frombuffer(b"".join(sigs), dtype=np.uint8).copy() if sigs else np.zeros(96, np.uint8),
        seed=seed,
    )


@dataclass
class PackedDeposits:
    """SoA form of one bls_gpu_verify_deposits call (bls_deposit_batch)."""

    pubkeys48: np.ndarray  # uint8[n * 48]
    withdrawal_credentials: np.ndarray  # uint8[n * 32]
    amounts: np.ndarray  # uint8[n * 8], little-endian Gwei
    signatures: np.ndarray  # uint8[n * 96]
    domain: np.ndarray  # uint8[32]
    n: int = 0
    seed: bytes | None = None


def pack_deposits(deposits, domain: bytes, seed: bytes | None = None) -> PackedDeposits:
    """deposits: list of (pubkey48, withdrawal_credentials32, amount: int, signature96), the
    fields of a DepositData; domain: the call's 32-byte deposit domain."""
    if len(domain) != 32:
        raise ValueError("the deposit domain is 32 bytes")
    pks, wcs, amts, sigs = [], [], [], []
    for pk, wc, amount, sig in deposits:
        pk, wc, sig = bytes(pk), bytes(wc), bytes(sig)
        if len(pk) != 48:
            raise ValueError(f"deposit pubkeys are 48 bytes (compressed G1), got {len(pk)}")
        if len(wc) != 32:
            raise ValueError(f"withdrawal credentials are 32 bytes, got {len(wc)}")
        if len(sig) != 96:
            raise ValueError(f"deposit signatures are 96 bytes (compressed G2), got {len(sig)}")
        amount = int(amount)
        if not 0 <= amount < 1 << 64:
            raise ValueError(f"a deposit amount is a uint64 (Gwei), got {amount}")
        pks.append(pk)
        wcs.append(wc)
        amts.append(amount.to_bytes(8, "little"))
        sigs.append(sig)

    def join(parts, size):
        return np.frombuffer(b"".join(parts), dtype=np.uint8).copy() if parts else np.zeros(size, np.uint8)

    return PackedDeposits(pubkeys48=join(pks, 48), withdrawal_credentials=join(wcs, 32), amounts=join(amts, 8),
                          signatures=join(sigs, 96), domain=_u8(domain), n=len(pks), seed=seed)


class GpuContext:
    def __init__(self, device: int = 0, high_priority: bool = False):
        """high_priority: the context's stream outranks normal contexts' queued kernels
        (bls_gpu_init_priority; the verifyOnMainThread latency lane)."""
        self.lib = load_library()
        ndev = self.lib.bls_gpu_device_count()
        if ndev <= device:
            raise NativeError(f"no HIP device {device} (visible: {ndev}); the verifier has no CPU fallback")
        h = ctypes.c_void_p()
        rc = self.lib.bls_gpu_init_priority(device, 1 if high_priority else 0, ctypes.byref(h))
        if rc != 0:
            msg = (self.lib.bls_gpu_init_error() or b"").decode() or f"bls_gpu_init_priority({device}) failed"
            raise (AdmissionError if rc == ERR_ADMISSION else NativeError)(msg)
        self._h = h
        self.device = device

    # -- lifecycle ------------------------------------------------------------
    def close(self) -> None:
        if self._h:
            self.lib.bls_gpu_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str):
        if rc < 0:
            msg = self.lib.bls_gpu_last_error(self._h)
            raise NativeError(f"{what}: {msg.decode() if msg else rc}")

    # -- pubkey table ---------------------------------------------------------
    def load_pubkeys(self, pks: bytes | np.ndarray, pk_len: int = 48) -> np.ndarray:
        arr = _u8(pks)
        n = arr.size // pk_len
        codes = np.zeros(max(n, 1), dtype=np.int32)
        rc = self.lib.bls_gpu_load_pubkeys(self._h, _ptr(arr), n, pk_len, _ptr(codes))
        self._check(rc, "bls_gpu_load_pubkeys")
        return codes[:n]

    def share_pubkeys(self, other: "GpuContext") -> None:
        """Use `other`'s key table instead of a replica of one's own (bls_gpu_share_pubkeys):
        this context must hold no keys and sit on the same device; afterwards a load through
        either context appends for both."""
        if not isinstance(other, GpuContext) or not other._h:
            raise NativeError("share_pubkeys: the other context is not open")
        self._check(self.lib.bls_gpu_share_pubkeys(self._h, other._h), "bls_gpu_share_pubkeys")

    def pubkeys_info(self) -> dict:
        """The key table this context uses (bls_pubkeys_info): table_id (equal for contexts
        that share a table), n_keys, capacity, comb_keys, n_contexts, device_bytes."""
        from ._abi import BlsPubkeysInfo

        info = BlsPubkeysInfo()
        self._check(self.lib.bls_gpu_pubkeys_info(self._h, ctypes.byref(info)), "bls_gpu_pubkeys_info")
        return {name: int(getattr(info, name)) for name, _ in BlsPubkeysInfo._fields_}

    def validate_pubkeys(self, pks: bytes | np.ndarray, pk_len: int = 48) -> np.ndarray:
        """KeyValidate codes (0 valid, else BLST-style code) for n keys (bls_gpu_validate_pubkeys)."""
        arr = _u8(pks)
        n = arr.size // pk_len
        codes = np.zeros(max(n, 1), dtype=np.int32)
        rc = self.lib.bls_gpu_validate_pubkeys(self._h, _ptr(arr), n, pk_len, _ptr(codes))
        self._check(rc, "bls_gpu_validate_pubkeys")
        return codes[:n]

    # -- verification -------------------------------------------------------------
    @staticmethod
    def _batch_struct(pb: PackedBatch):
        # cached on the batch: the view points at the batch's arrays, so edits in place
        # are seen; a caller that replaces one of them must build a new PackedBatch
        if pb._cstruct is not None:
            return pb._cstruct
        keep = []
        b = BlsBatch()
        b.n_sets = pb.n_sets
        b.n_reqs = pb.n_reqs
        for field in ("req_set_offsets", "req_batchable", "messages", "signatures", "pubkeys", "set_pk_offsets",
                      "pk_indices", "signature_lens"):
            a = getattr(pb, field)
            if a is not None:
                a = np.ascontiguousarray(a)
                keep.append(a)
            setattr(b, field, _ptr(a))
        seed_buf = None
        if pb.seed is not None:
            seed_buf = ctypes.create_string_buffer(bytes(pb.seed), 32)
            b.seed = ctypes.cast(seed_buf, ctypes.c_void_p)
        keep.append(seed_buf)
        pb._cstruct = (b, keep)
        return b, keep

    def verify_packed(self, pb: PackedBatch) -> tuple[np.ndarray, BlsStats]:
        b, _keep = self._batch_struct(pb)
        verdicts = np.zeros(max(pb.n_reqs, 1), dtype=np.int32)
        stats = BlsStats()
        rc = self.lib.bls_gpu_verify(self._h, ctypes.byref(b), _ptr(verdicts), ctypes.byref(stats))
        self._check(rc, "bls_gpu_verify")
        return verdicts[: pb.n_reqs], stats

    # -- committee groups -----------------------------------------------------------
    def set_committee_group(self, group: int, committees) -> None:
        """Register (replace) committee group `group` (0..7): `committees` is a list of member
        lists of table indices, in committee order, duplicates allowed; an empty list drops
        the group (bls_gpu_set_committee_group).  Raises NativeError, the group unchanged,
        for a member past the table, an empty committee or a group past the slots."""
        offs, mem = [0], []
        for c in committees:
            mem.extend(int(i) for i in c)
            offs.append(len(mem))
        o = np.array(offs, dtype=np.uint32)
        m = np.array(mem if mem else [0], dtype=np.uint32)
        rc = self.lib.bls_gpu_set_committee_group(self._h, group, len(offs) - 1, _ptr(o), _ptr(m))
        self._check(rc, "bls_gpu_set_committee_group")

    def committee_group_info(self, group: int) -> dict:
        """n_committees, n_members and device_bytes of group `group` (all 0: not registered)."""
        info = BlsCommitteeInfo()
        self._check(self.lib.bls_gpu_committee_group_info(self._h, group, ctypes.byref(info)),
                    "bls_gpu_committee_group_info")
        return {name: int(getattr(info, name)) for name, _ in BlsCommitteeInfo._fields_}

    @staticmethod
    def _committee_struct(set_committee, set_bits_off, bits):
        keep = [np.ascontiguousarray(set_committee, dtype=np.uint32), np.ascontiguousarray(set_bits_off, dtype=np.uint32),
                np.ascontiguousarray(bits, dtype=np.uint8)]
        cs = BlsCommitteeSets()
        cs.set_committee, cs.set_bits_off, cs.bits = (_ptr(a) for a in keep)
        return cs, keep

    def verify_committees_packed(self, pb: PackedBatch) -> tuple[np.ndarray, BlsStats]:
        """bls_gpu_verify_committees for a batch packed from requests that hold committee
        sets (pack_requests); one without any goes to bls_gpu_verify as verify_packed does."""
        if pb.set_committee is None:
            return self.verify_packed(pb)
        b, _keep = self._batch_struct(pb)
        cs, _keep2 = self._committee_struct(pb.set_committee, pb.set_bits_off, pb.bits)
        verdicts = np.zeros(max(pb.n_reqs, 1), dtype=np.int32)
        stats = BlsStats()
        rc = self.lib.bls_gpu_verify_committees(self._h, ctypes.byref(b), ctypes.byref(cs), _ptr(verdicts),
                                                ctypes.byref(stats))
        self._check(rc, "bls_gpu_verify_committees")
        return verdicts[: pb.n_reqs], stats

    def aggregate_committee_bits(self, sets) -> tuple[list[bytes], np.ndarray]:
        """sets: list of ((group, index), bits).  The aggregate key of each committee's members
        at the set bits, as aggregate_pubkeys gives it for the expanded index list: 96-byte
        uncompressed keys and codes (bls_gpu_aggregate_committee_bits)."""
        n = len(sets)
        refs = [COMMITTEE_REF(int(g), int(i)) for (g, i), _ in sets]
        offs = [0]
        for _, bt in sets:
            offs.append(offs[-1] + len(bytes(bt)))
        cs, _keep = self._committee_struct(np.array(refs if refs else [0], dtype=np.uint32), np.array(offs, dtype=np.uint32),
                                           np.frombuffer(b"".join(bytes(bt) for _, bt in sets) or b"\0", dtype=np.uint8))
        out = np.zeros(96 * max(n, 1), dtype=np.uint8)
        codes = np.zeros(max(n, 1), dtype=np.int32)
        rc = self.lib.bls_gpu_aggregate_committee_bits(self._h, ctypes.byref(cs), n, _ptr(out), _ptr(codes))
        self._check(rc, "bls_gpu_aggregate_committee_bits")
        raw = out.tobytes()
        return [raw[96 * i: 96 * i + 96] for i in range(n)], codes[:n]

    # -- spans: sets over several committees under one field ------------------------
    @staticmethod
    def _span_struct(set_span_off, span_refs, set_bits_off, bits):
        keep = [np.ascontiguousarray(set_span_off, dtype=np.uint32), np.ascontiguousarray(span_refs, dtype=np.uint32),
                np.ascontiguousarray(set_bits_off, dtype=np.uint32), np.ascontiguousarray(bits, dtype=np.uint8)]
        ss = BlsSpanSets()
        ss.set_span_off, ss.span_refs, ss.set_bits_off, ss.bits = (_ptr(a) for a in keep)
        return ss, keep

    def verify_spans_packed(self, pb: PackedBatch) -> tuple[np.ndarray, BlsStats]:
        """bls_gpu_verify_spans for a batch packed from requests that hold span sets
        (pack_requests); one without any goes where verify_committees_packed sends it."""
        if pb.set_span_off is None:
            return self.verify_committees_packed(pb)
        b, _keep = self._batch_struct(pb)
        ss, _keep2 = self._span_struct(pb.set_span_off, pb.span_refs, pb.set_bits_off, pb.bits)
        verdicts = np.zeros(max(pb.n_reqs, 1), dtype=np.int32)
        stats = BlsStats()
        rc = self.lib.bls_gpu_verify_spans(self._h, ctypes.byref(b), ctypes.byref(ss), _ptr(verdicts),
                                           ctypes.byref(stats))
        self._check(rc, "bls_gpu_verify_spans")
        return verdicts[: pb.n_reqs], stats

    def aggregate_spans(self, sets) -> tuple[list[bytes], np.ndarray]:
        """sets: list of ([(group, index), ...], bits).  The aggregate key of each span -- the
        members of its committees concatenated in order, at the set bits -- as aggregate_pubkeys
        gives it for the expanded index list: 96-byte uncompressed keys and codes
        (bls_gpu_aggregate_spans)."""
        n = len(sets)
        refs, soffs, boffs = [], [0], [0]
        for segs, bt in sets:
            refs.extend(COMMITTEE_REF(int(g), int(i)) for g, i in segs)
            soffs.append(len(refs))
            boffs.append(boffs[-1] + len(bytes(bt)))
        ss, _keep = self._span_struct(np.array(soffs, dtype=np.uint32), np.array(refs if refs else [0], dtype=np.uint32),
                                      np.array(boffs, dtype=np.uint32),
                                      np.frombuffer(b"".join(bytes(bt) for _, bt in sets) or b"\0", dtype=np.uint8))
        out = np.zeros(96 * max(n, 1), dtype=np.uint8)
        codes = np.zeros(max(n, 1), dtype=np.int32)
        rc = self.lib.bls_gpu_aggregate_spans(self._h, ctypes.byref(ss), n, _ptr(out), _ptr(codes))
        self._check(rc, "bls_gpu_aggregate_spans")
        raw = out.tobytes()
        return [raw[96 * i: 96 * i + 96] for i in range(n)], codes[:n]

    def verify_many(self, pbs: list[PackedBatch]) -> tuple[list[np.ndarray], BlsStats]:
        """Several worker messages in one submission (bls_gpu_verify_many): per-message
        verdict arrays (each as verify_packed would return it) and the totals."""
        structs, keep = (BlsBatch * max(len(pbs), 1))(), []
        for k, pb in enumerate(pbs):
            b, kp = self._batch_struct(pb)
            structs[k] = b
            keep.append(kp)
        total = sum(pb.n_reqs for pb in pbs)
        verdicts = np.zeros(max(total, 1), dtype=np.int32)
        stats = BlsStats()
        rc = self.lib.bls_gpu_verify_many(self._h, structs, len(pbs), _ptr(verdicts), ctypes.byref(stats))
        self._check(rc, "bls_gpu_verify_many")
        out, off = [], 0
        for pb in pbs:
            out.append(verdicts[off: off + pb.n_reqs])
            off += pb.n_reqs
        return out, stats

    def verify_same_message_packed(self, ps: PackedSameMsg) -> tuple[int, np.ndarray, BlsStats]:
        """bls_gpu_verify_same_message as it is: (return code, n_sets verdicts, stats)."""
        b = BlsSameMsgBatch()
        b.n_jobs, b.n_sets = ps.n_jobs, ps.n_sets
        keep = [np.ascontiguousarray(getattr(ps, f)) for f in ("job_set_offsets", "messages", "pk_indices",
                                                                "signatures")]
        b.job_set_offsets, b.messages, b.pk_indices, b.signatures = (_ptr(a) for a in keep)
        seed_buf = None
        if ps.seed is not None:
            seed_buf = ctypes.create_string_buffer(bytes(ps.seed), 32)
            b.seed = ctypes.cast(seed_buf, ctypes.c_void_p)
        verdicts = np.zeros(max(ps.n_sets, 1), dtype=np.int32)
        stats = BlsStats()
        rc = self.lib.bls_gpu_verify_same_message(self._h, ctypes.byref(b), _ptr(verdicts), ctypes.byref(stats))
        return rc, verdicts[: ps.n_sets], stats

    def verify_same_message(self, jobs, seed: bytes | None = None) -> tuple[list[np.ndarray], BlsStats]:
        """verifySignatureSetsSameMessage for several jobs in one native call
        (bls_gpu_verify_same_message).  jobs: list of (message32, [table index...],
        [sig96...]); each job is ONE random-scalar batch over its sets.  Returns one int32
        array per job -- per set 1 valid, 0 invalid, -code an error under the one-set rules
        (all 1 when the job's batch passes) -- and the call's stats."""
        ps = jobs if isinstance(jobs, PackedSameMsg) else pack_same_message(jobs, seed)
        rc, verdicts, stats = self.verify_same_message_packed(ps)
        self._check(rc, "bls_gpu_verify_same_message")
        off = ps.job_set_offsets
        return [verdicts[int(off[j]): int(off[j + 1])] for j in range(ps.n_jobs)], stats

    def verify_deposits_packed(self, pd: PackedDeposits) -> tuple[int, np.ndarray, BlsStats]:
        """bls_gpu_verify_deposits as it is: (return code, n verdicts 1 / 0 / -code, stats)."""
        b = BlsDepositBatch()
        b.n = pd.n
        keep = [np.ascontiguousarray(getattr(pd, f)) for f in ("pubkeys48", "withdrawal_credentials", "amounts",
                                                                "signatures", "domain")]
        b.pubkeys48, b.withdrawal_credentials, b.amounts, b.signatures, b.domain = (_ptr(a) for a in keep)
        seed_buf = None
        if pd.seed is not None:
            seed_buf = ctypes.create_string_buffer(bytes(pd.seed), 32)
            b.seed = ctypes.cast(seed_buf, ctypes.c_void_p)
        verdicts = np.zeros(max(pd.n, 1), dtype=np.int32)
        stats = BlsStats()
        rc = self.lib.bls_gpu_verify_deposits(self._h, ctypes.byref(b), _ptr(verdicts), ctypes.byref(stats))
        return rc, verdicts[: pd.n], stats

    def partial(self, pb: PackedBatch, set_index_base: int):
        """Miller-loop partial of this shard of a sharded call (bls_gpu_partial):
        (576 opaque bytes or None on an error, status 0 / -code, (class, shard-local set
        index) of the error or None, stats)."""
        if pb.seed is None:
            raise ValueError("a sharded call needs the call's shared 32-byte seed")
        b, _keep = self._batch_struct(pb)
        out = np.zeros(576, dtype=np.uint8)
        status = ctypes.c_int32(0)
        err = np.zeros(2, dtype=np.uint32)
        stats = BlsStats()
        rc = self.lib.bls_gpu_partial(self._h, ctypes.byref(b), set_index_base, _ptr(out), ctypes.byref(status),
                                      _ptr(err), ctypes.byref(stats))
        self._check(rc, "bls_gpu_partial")
        if status.value == 0:
            return out.tobytes(), 0, None, stats
        return None, status.value, (int(err[0]), int(err[1])), stats

    def final_check(self, partials: list[bytes]) -> bool:
        """FE(prod partials) == 1: the one final exponentiation of a sharded call."""
        buf = _u8(b"".join(partials))
        v = ctypes.c_int32(-1)
        rc = self.lib.bls_gpu_final_check(self._h, _ptr(buf), len(partials), ctypes.byref(v))
        self._check(rc, "bls_gpu_final_check")
        return v.value == 1

    # -- standalone primitives (parity tests, fixtures) ---------------------------
    def aggregate_pubkeys(self, index_lists) -> tuple[list[bytes], np.ndarray]:
        offs = [0]
        idx = []
        for lst in index_lists:
            idx.extend(int(i) for i in lst)
            offs.append(len(idx))
        n = len(index_lists)
        o = np.array(offs, dtype=np.uint32)
        ix = np.array(idx if idx else [0], dtype=np.uint32)
        out = np.zeros(96 * max(n, 1), dtype=np.uint8)
        codes = np.zeros(max(n, 1), dtype=np.int32)
        rc = self.lib.bls_gpu_aggregate_pubkeys(self._h, _ptr(o), _ptr(ix), n, _ptr(out), _ptr(codes))
        self._check(rc, "bls_gpu_aggregate_pubkeys")
        raw = out.tobytes()
        return [raw[96 * i: 96 * i + 96] for i in range(n)], codes[:n]

    def hash_to_g2(self, msgs: bytes | np.ndarray) -> np.ndarray:
        m = _u8(msgs)
        n = m.size // 32
        out = np.zeros(192 * max(n, 1), dtype=np.uint8)
        self._check(self.lib.bls_gpu_hash_to_g2(self._h, _ptr(m), n, _ptr(out)), "bls_gpu_hash_to_g2")
        return out[: 192 * n].reshape(n, 192)

    def ssz_roots(self, kind: int, objs: bytes | np.ndarray, domains: bytes | np.ndarray | None = None) -> np.ndarray:
        """computeSigningRoot over n serialized objects of one SSZ kind (bls_gpu_ssz_roots;
        signingRoot.ts:7-13): n x 32 signing roots, or the objects' hash_tree_roots when
        domains is None.  domains: one 32-byte domain for all, or 32 bytes per object."""
        o = _u8(objs)
        size = kind & 0xFF
        if o.size % size:
            raise ValueError(f"objects are {size} bytes each, got {o.size} bytes")
        n = o.size // size
        d, stride = None, 0
        if domains is not None:
            d = _u8(domains)
            if d.size == 32:
                stride = 0
            elif d.size == 32 * n:
                stride = 32
            else:
                raise ValueError("domains: 32 bytes, or 32 bytes per object")
        out = np.zeros(32 * max(n, 1), dtype=np.uint8)
        rc = self.lib.bls_gpu_ssz_roots(self._h, kind, _ptr(o) if n else None, n, _ptr(d), stride, _ptr(out))
        self._check(rc, "bls_gpu_ssz_roots")
        return out[: 32 * n].reshape(n, 32)

    def g2_decompress(self, sigs96: bytes | np.ndarray, validate: bool = True) -> tuple[np.ndarray, np.ndarray]:
        """Signature.fromBytes(b, affine, validate) for n 96-byte signatures:
        (n x 192 uncompressed bytes, n codes) (bls_gpu_g2_decompress)."""
        s = _u8(sigs96)
        n = s.size // 96
        out = np.zeros(192 * max(n, 1), dtype=np.uint8)
        codes = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.lib.bls_gpu_g2_decompress(self._h, _ptr(s), n, 1 if validate else 0, _ptr(out), _ptr(codes)),
                    "bls_gpu_g2_decompress")
        return out[: 192 * n].reshape(n, 192), codes[:n]

    def aggregate_signatures(self, sig_lists) -> tuple[list[bytes], np.ndarray]:
        """Signature.aggregate over lists of 96-byte signatures (each decoded with
        validate=true): (compressed sums, codes) (bls_gpu_aggregate_signatures)."""
        offs, flat = [0], []
        for lst in sig_lists:
            for sig in lst:
                b = bytes(sig)
                if len(b) != 96:
                    raise ValueError("signatures are 96 bytes (compressed G2)")
                flat.append(b)
            offs.append(len(flat))
        n_lists = len(sig_lists)
        o = np.array(offs, dtype=np.uint32)
        buf = np.frombuffer(b"".join(flat), dtype=np.uint8).copy() if flat else np.zeros(96, np.uint8)
        out = np.zeros(96 * max(n_lists, 1), dtype=np.uint8)
        codes = np.zeros(max(n_lists, 1), dtype=np.int32)
        self._check(self.lib.bls_gpu_aggregate_signatures(self._h, _ptr(buf), _ptr(o), n_lists, _ptr(out),
                                                          _ptr(codes)), "bls_gpu_aggregate_signatures")
        raw = out.tobytes()
        return [raw[96 * i: 96 * i + 96] for i in range(n_lists)], codes[:n_lists]

    def sk_to_pk(self, sks: bytes | np.ndarray) -> np.ndarray:
        s = _u8(sks)
        n = s.size // 32
        out = np.zeros(48 * max(n, 1), dtype=np.uint8)
        self._check(self.lib.bls_gpu_sk_to_pk(self._h, _ptr(s), n, _ptr(out)), "bls_gpu_sk_to_pk")
        return out[: 48 * n].reshape(n, 48)

    # ORed into every set_debug_flags call (tests run a whole module once per path)
    base_debug_flags = 0

    def set_debug_flags(self, flags: int) -> None:
        self._check(self.lib.bls_gpu_set_debug_flags(self._h, flags | self.base_debug_flags),
                    "bls_gpu_set_debug_flags")

    def group_test_counts(self) -> list[int]:
        """The group-test rounds of the last verify pass (bls_gpu_group_test_counts): chunks
        group-tested, of those taking the whole's value from the chunk check, pass A's tests
        and chunks decided, pass B's, pass C's tests, and whether pass A's sums did not fit."""
        out = (ctypes.c_uint32 * 8)()
        self._check(self.lib.bls_gpu_group_test_counts(self._h, out), "bls_gpu_group_test_counts")
        return [int(x) for x in out]

    def mad_peak(self) -> tuple[float, float]:
        """Measured v_mad_u64_u32 rate (MAD/s) and the probe's duration (ms)."""
        rate, ms = ctypes.c_double(), ctypes.c_double()
        self._check(self.lib.bls_gpu_mad_peak(self._h, ctypes.byref(rate), ctypes.byref(ms)), "bls_gpu_mad_peak")
        return rate.value, ms.value

    def fp_mul_test(self, a: bytes, b: bytes) -> bytes:
        n = len(a) // 48
        out = ctypes.create_string_buffer(48 * max(n, 1))
        self._check(self.lib.bls_gpu_fp_mul_test(self._h, a, b, n, out), "bls_gpu_fp_mul_test")
        return out.raw[: 48 * n]

    def field_op_shape(self, op: int) -> tuple[int, int]:
        """(words per input record, words per output record) of a field-op self-test op"""
        iw, ow = ctypes.c_uint32(), ctypes.c_uint32()
        if self.lib.bls_gpu_field_op_shape(op, ctypes.byref(iw), ctypes.byref(ow)) != 0:
            raise NativeError(f"bls_gpu_field_op_shape: unknown field op {op:#x}")
        return iw.value, ow.value

    def field_op_test(self, op: int, records: np.ndarray) -> np.ndarray:
        """One field primitive per record on raw 32-bit words (include/lodestar_bls.h
        bls_gpu_field_op_test): records is (n, in_words) uint32, the result (n, out_words)."""
        iw, ow = self.field_op_shape(op)
        rec = np.ascontiguousarray(records, dtype=np.uint32)
        if rec.ndim != 2 or rec.shape[1] != iw:
            raise ValueError(f"field op {op:#x} takes records of {iw} words, got {rec.shape}")
        n = rec.shape[0]
        out = np.zeros((max(n, 1), ow), dtype=np.uint32)
        self._check(self.lib.bls_gpu_field_op_test(self._h, op, _ptr(rec), n, _ptr(out)), "bls_gpu_field_op_test")
        return out[:n]

    def curve_op_shape(self, op: int) -> tuple[int, int]:
        """(words per input record, words per output record) of a curve-op self-test op"""
        iw, ow = ctypes.c_uint32(), ctypes.c_uint32()
        if self.lib.bls_gpu_curve_op_shape(op, ctypes.byref(iw), ctypes.byref(ow)) != 0:
            raise NativeError(f"bls_gpu_curve_op_shape: unknown curve op {op:#x} (or not in this flavour)")
        return iw.value, ow.value

    def curve_op_test(self, op: int, records: np.ndarray) -> np.ndarray:
        """One curve-level function of the verify path per record on Montgomery-form words
        (include/lodestar_bls.h bls_gpu_curve_op_test): records is (n, in_words) uint32, the
        result (n, out_words)."""
        iw, ow = self.curve_op_shape(op)
        rec = np.ascontiguousarray(records, dtype=np.uint32)
        if rec.ndim != 2 or rec.shape[1] != iw:
            raise ValueError(f"curve op {op:#x} takes records of {iw} words, got {rec.shape}")
        n = rec.shape[0]
        out = np.zeros((max(n, 1), ow), dtype=np.uint32)
        self._check(self.lib.bls_gpu_curve_op_test(self._h, op, _ptr(rec), n, _ptr(out)), "bls_gpu_curve_op_test")
        return out[:n]

    def tower_op_shape(self, op: int) -> tuple[int, int]:
        """(words per input record, words per output record) of a tower-op self-test op"""
        iw, ow = ctypes.c_uint32(), ctypes.c_uint32()
        if self.lib.bls_gpu_tower_op_shape(op, ctypes.byref(iw), ctypes.byref(ow)) != 0:
            raise NativeError(f"bls_gpu_tower_op_shape: unknown tower op {op:#x} (or not in this flavour)")
        return iw.value, ow.value

    def tower_op_test(self, op: int, records: np.ndarray) -> np.ndarray:
        """One Fp6 / Fp12 tower function of the verify path per record on Montgomery-form words
        (include/lodestar_bls.h bls_gpu_tower_op_test): records is (n, in_words) uint32, the
        result (n, out_words)."""
        iw, ow = self.tower_op_shape(op)
        rec = np.ascontiguousarray(records, dtype=np.uint32)
        if rec.ndim != 2 or rec.shape[1] != iw:
            raise ValueError(f"tower op {op:#x} takes records of {iw} words, got {rec.shape}")
        n = rec.shape[0]
        out = np.zeros((max(n, 1), ow), dtype=np.uint32)
        self._check(self.lib.bls_gpu_tower_op_test(self._h, op, _ptr(rec), n, _ptr(out)), "bls_gpu_tower_op_test")
        return out[:n]

    def coop_run_test(self, name: str, frames: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """Program `name` of the loaded table run once per frame: frames is (n_frames,
        n_slots, 12) uint32 raw Fp limbs; returns the raw frames after the run and the
        zero-check flag word of each."""
        fr = np.ascontiguousarray(frames, dtype=np.uint32)
        if fr.ndim != 3 or fr.shape[2] != 12:
            raise ValueError(f"frames must be (n_frames, n_slots, 12) uint32, got {fr.shape}")
        out = np.zeros_like(fr)
        flags = np.zeros(max(fr.shape[0], 1), dtype=np.uint32)
        self._check(self.lib.bls_gpu_coop_run_test(self._h, name.encode(), _ptr(fr), fr.shape[0], fr.shape[1],
                                                   _ptr(out), _ptr(flags)), "bls_gpu_coop_run_test")
        return out, flags[: fr.shape[0]]

    def fpm_bench(self, lanes: int, iters: int) -> tuple[float, float]:
        ns, rate = ctypes.c_double(), ctypes.c_double()
        self._check(self.lib.bls_gpu_fpm_bench(self._h, lanes, iters, ctypes.byref(ns), ctypes.byref(rate)),
                    "bls_gpu_fpm_bench")
        return ns.value, rate.value

    def kernel_probe(self, name: str, lanes: int, reps: int) -> float:
        """Wall ms of `reps` launches of the design probe `name` over `lanes` lanes
        (kernels/k_probe.hip)."""
        ms = ctypes.c_double()
        self._check(self.lib.bls_gpu_kernel_probe(self._h, name.encode(), lanes, reps, ctypes.byref(ms)),
                    "bls_gpu_kernel_probe")
        return ms.value

    def coop_probe(self, name: str, blocks: int, reps: int, n_stamps: int = 0):
        """(us per step, ms total[, per-step s_memtime stamps of one run])"""
        us, ms = ctypes.c_double(), ctypes.c_double()
        stamps = np.zeros(n_stamps, dtype=np.uint64) if n_stamps else None
        self._check(self.lib.bls_gpu_coop_probe(self._h, name.encode(), blocks, reps, ctypes.byref(us),
                                                ctypes.byref(ms), _ptr(stamps)), "bls_gpu_coop_probe")
        if stamps is not None:
            return us.value, ms.value, stamps
        return us.value, ms.value

    def sign(self, sks: bytes | np.ndarray, msgs: bytes | np.ndarray) -> np.ndarray:
        s, m = _u8(sks), _u8(msgs)
        n = s.size // 32
        out = np.zeros(96 * max(n, 1), dtype=np.uint8)
        self._check(self.lib.bls_gpu_sign(self._h, _ptr(s), _ptr(m), n, _ptr(out)), "bls_gpu_sign")
        return out[: 96 * n].reshape(n, 96)
