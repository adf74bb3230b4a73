"""Deposit signature verification (bls_gpu_verify_deposits, include/lodestar_bls.h).

processDeposit (state-transition/src/block/processDeposit.ts:48-65) checks the deposit of
an unknown validator on its own -- KeyValidate of the untrusted 48-byte key, the signature
decoded with validation, verify over the DepositMessage signing root -- and skips it when
any step fails or throws.  Here one native call checks a list of deposits, each given by
the four fields of its DepositData; the keys never enter the device table and the
signing roots are computed on the GPU.

A deposit is `(pubkey48, withdrawal_credentials32, amount: int, signature96)`.
"""
from __future__ import annotations

import hashlib

import numpy as np

from . import _abi
from ._abi import CODE_INVALID_SIZE
from .native import GpuContext, NativeError, PackedDeposits, pack_deposits

DOMAIN_DEPOSIT = bytes.fromhex("03000000")


def _sha(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def deposit_domain(fork_version: bytes, genesis_validators_root: bytes = bytes(32)) -> bytes:
    """compute_domain(DOMAIN_DEPOSIT, fork_version, genesis_validators_root): the domain
    type followed by the first 28 bytes of hash_tree_root(ForkData) (util/domain.ts:27-45).
    Deposits are valid across forks, so the root is the zero root and the version the
    genesis fork version (processDeposit.ts:52)."""
    fork_version, genesis_validators_root = bytes(fork_version), bytes(genesis_validators_root)
    if len(fork_version) != 4 or len(genesis_validators_root) != 32:
        raise ValueError("fork_version is 4 bytes, genesis_validators_root 32")
    fork_data_root = _sha(fork_version.ljust(32, b"\0") + genesis_validators_root)
    return DOMAIN_DEPOSIT + fork_data_root[:28]


def split_deposits(deposits: list, cap: int | None = None) -> list[list]:
    """the list in parts of at most `cap` deposits (BLS_DEPOSITS_MAX_CALL), in order"""
    cap = _abi.DEPOSITS_MAX_CALL if cap is None else cap
    return [deposits[i: i + cap] for i in range(0, len(deposits), cap)]


def screen_deposits(deposits) -> tuple[list, list[int]]:
    """(the deposits the native call takes, their positions): a signature of another
    length than 96 bytes cannot be a signature, so that deposit is invalid without a GPU
    call (BLST_INVALID_SIZE in the reference's try block); every other field length is
    the caller's error and raises in pack_deposits."""
    deposits = [tuple(d) for d in deposits]
    keep = [k for k, d in enumerate(deposits) if len(bytes(d[3])) == 96]
    return [deposits[k] for k in keep], keep


def verify_deposit_codes(ctx: GpuContext, deposits, fork_version: bytes | None = None, domain: bytes | None = None,
                         seed: bytes | None = None) -> np.ndarray:
    """One code per deposit: 1 valid, 0 invalid, -code when a step of the reference's try
    block throws (the order of include/lodestar_bls.h bls_gpu_verify_deposits;
    -BLS_CODE_INVALID_SIZE for a signature that is not 96 bytes).  Give the fork version
    (the domain is computed here) or the 32-byte domain itself.  Lists above
    BLS_DEPOSITS_MAX_CALL go to the GPU in parts of at most that many."""
    if (fork_version is None) == (domain is None):
        raise ValueError("give fork_version or domain")
    dom = bytes(domain) if domain is not None else deposit_domain(fork_version)
    deposits = list(deposits)
    out = np.full(len(deposits), -CODE_INVALID_SIZE, dtype=np.int32)
    taken, pos = screen_deposits(deposits)
    off = 0
    for part in split_deposits(taken):
        rc, v, _ = ctx.verify_deposits_packed(pack_deposits(part, dom, seed))
        if rc < 0:
            msg = ctx.lib.bls_gpu_last_error(ctx._h)
            raise NativeError(f"bls_gpu_verify_deposits: {msg.decode() if msg else rc}")
        out[pos[off: off + len(part)]] = v
        off += len(part)
    return out


def verify_deposits(ctx: GpuContext, deposits, fork_version: bytes) -> list[bool]:
    """True per deposit whose signature verifies; an invalid deposit is False, never an
    exception (processDeposit skips it)."""
    return [int(c) == 1 for c in verify_deposit_codes(ctx, deposits, fork_version=fork_version)]


__all__ = ["DOMAIN_DEPOSIT", "PackedDeposits", "deposit_domain", "pack_deposits", "screen_deposits",
           "split_deposits", "verify_deposit_codes", "verify_deposits"]
