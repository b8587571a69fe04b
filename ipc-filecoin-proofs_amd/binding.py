"""ctypes binding of ``libipcfp.so`` (C ABI: ``include/ipcfp.h``).

Plumbing only.  Every method forwards to one C entry point; numpy arrays carry the
host buffers.  No algorithm lives here and nothing falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

__all__ = [
    "ABI_VERSION",
    "SCAN_PHASE_RECEIPTS",
    "SCAN_PHASE_EVENTS",
    "MAX_SCAN_SPECS",
    "MAX_SCAN_TIPSETS",
    "merge_scan_status",
    "host_register",
    "ingest_buffer",
    "host_unregister",
    "Engine",
    "EventProofSpec",
    "STORAGE_SPEC_DTYPE",
    "Comm",
    "shard_range",
    "witness_cut_host",
    "route_event_claims",
    "comm_unique_id",
    "allgather_segments",
    "EngineError",
    "Witness",
    "Bundle",
    "bundle_check_json",
    "bundle_claims_json",
    "pack_event_proofs",
    "pack_storage_proofs",
    "GEN_STORAGE_DTYPE",
    "lib_path",
    "load_library",
    "ST",
    "CID_OK",
    "CID_MISMATCH",
    "CID_UNCHECKED",
    "KERNEL_IDS",
    "pack_event_claims",
    "PackedWitnessTables",
    "STD_CID_PREFIX",
    "compact_event_claims",
    "COMPACT_DTYPE",
    "GROUP_DTYPE",
    "pack_storage_claims",
    "SCLAIM_DTYPE",
    "compact_storage_claims",
    "expand_storage_claims",
    "StorageColumns",
    "GeneratedEvents",
    "unpack_event_claims",
    "UnpackedEvents",
    "GeneratedStorageClaims",
    "unpack_storage_claims",
    "UnpackedStorage",
    "StorageProofStruct",
    "EventProofStruct",
    "cid_from_string",
    "cid_to_string",
    "pack_cids",
    "CLAIM_DTYPE",
    "TIPSET_DTYPE",
    "TipsetRefs",
    "cid_slot",
    "cid_slots",
    "LOC_DTYPE",
    "MATCH_DTYPE",
]

_HERE = os.path.dirname(os.path.abspath(__file__))

CID_MISMATCH, CID_OK, CID_UNCHECKED = 0, 1, 2
CID_SLOT = 40

KERNEL_IDS = {
    "blake2b_cid": 0,
    "keccak256": 1,
    "sha256": 2,
    "cid_index": 3,
    "amt_get": 4,
    "event_scan": 5,
    "hamt_get": 6,
    "replay": 7,
    "event_verify": 8,
    "storage_verify": 9,
    "exec_order": 10,
    "blake2b_raw": 11,
    "base64": 12,
    "allgather": 13,
    "tipset_prologue": 14,
    "amt_walk": 15,
    "claim_sizes": 16,
    "claim_scan": 17,
    "claim_fill": 18,
    "sgen_runs": 19,
    "sgen_specs": 20,
    "sgen_records": 21,
    "scan_multi_count": 22,
    "scan_multi_fill": 23,
    "scan_multi_tail": 24,
    "scan_tipsets": 25,
    "gen_tipsets": 26,
    "claim_text": 27,
}

MAX_SCAN_SPECS = 1024
MAX_SCAN_TIPSETS = 4096


class ST:
    """ipcfp_status_t values (include/ipcfp.h)."""

    FALSE = 0
    TRUE = 1
    FALSE_UNTRUSTED_PARENT = 2
    FALSE_UNTRUSTED_CHILD = 3
    FALSE_PARENTS_MISMATCH = 4
    FALSE_CHILD_EPOCH = 5
    FALSE_PARENT_EPOCH = 6
    FALSE_MSG_NOT_IN_EXEC = 7
    FALSE_EXEC_INDEX = 8
    FALSE_NO_RECEIPT = 9
    FALSE_NO_EVENTS_ROOT = 10
    FALSE_NO_EVENT = 11
    FALSE_EMITTER = 12
    FALSE_NOT_EVM_LOG = 13
    FALSE_TOPIC_COUNT = 14
    FALSE_TOPIC = 15
    FALSE_DATA = 16
    FALSE_FILTER = 17
    FALSE_STATE_ROOT = 18
    FALSE_ACTOR_STATE = 19
    FALSE_STORAGE_ROOT = 20
    FALSE_VALUE = 21
    NOT_FOUND = 32
    ERR = 64
    ERR_MISSING_BLOCK = 65
    ERR_DECODE = 66
    ERR_TXMETA_MISMATCH = 67
    ERR_ACTOR_NOT_FOUND = 68
    ERR_BAD_CLAIM = 69
    ERR_MAX_DEPTH = 70
    ERR_EMPTY_PARENTS = 71

    @staticmethod
    def is_err(s: int) -> bool:
        return s >= 64

    @staticmethod
    def is_true(s: int) -> bool:
        return s == 1


VALUE_KINDS = {"cid": 0, "receipt": 1, "stamped_event": 2, "actor_state": 3, "vec_u8": 4, "any": 5}
LOC_DTYPE = np.dtype([("block", np.uint32), ("off", np.uint32), ("len", np.uint32)])
MAX_PARENTS = 32
# (`more_parents`: host address of the slots of parents[MAX_PARENTS ..] when n_parents > MAX_PARENTS — TipsetRefs keeps them alive)
TIPSET_DTYPE = np.dtype([("flags", np.uint32), ("n_parents", np.uint32), ("child", np.uint8, (CID_SLOT,)),
                         ("parents", np.uint8, (MAX_PARENTS, CID_SLOT)), ("more_parents", np.uint64)])


class TipsetRefs(np.ndarray):
    """ipcfp_tipset_ref_t[] that owns the arrays its `more_parents` pointers name (tipset keys of more than MAX_PARENTS blocks)."""

    def __array_finalize__(self, obj):
        self._keep = getattr(obj, "_keep", [])


def cid_slot(cid: bytes) -> np.ndarray:
    """A binary CID of any length as its 40-byte slot: zero padded, or — longer than the slot — FOLDED
    (ff | len | blake2b-256(cid); include/ipcfp.h "CIDs", ipcfp_cid_to_slot)."""
    out = np.zeros(CID_SLOT, dtype=np.uint8)
    raw = np.frombuffer(bytes(cid), dtype=np.uint8)
    rc = load_library().ipcfp_cid_to_slot(_p(raw), len(raw), _p(out))
    if rc < 0:
        raise EngineError(f"cid_slot: not a CID ({rc})")
    return out


def cid_slots(cids) -> np.ndarray:
    """[binary CID, …] → u8[n, 40] (each through cid_slot)."""
    out = np.zeros((len(cids), CID_SLOT), dtype=np.uint8)
    for i, c in enumerate(cids):
        c = bytes(c)
        out[i] = cid_slot(c) if len(c) > CID_SLOT else np.frombuffer(c.ljust(CID_SLOT, b"\0"), dtype=np.uint8)
    return out
CLAIM_DTYPE = np.dtype([("parent_epoch", np.int64), ("child_epoch", np.int64), ("exec_index", np.uint64),
                        ("event_index", np.uint64), ("emitter", np.uint64), ("message_cid", np.uint8, (CID_SLOT,)),
                        ("tipset", np.uint32), ("flags", np.uint32), ("n_topics", np.uint32),
                        ("topics_off", np.uint32), ("data_off", np.uint32), ("data_len", np.uint32)])
ABI_VERSION = 3  # == IPCFP_ABI_VERSION of include/ipcfp.h (tests/test_abi_symbols.py holds the three together)
SCAN_PHASE_RECEIPTS, SCAN_PHASE_EVENTS = 1, 2


def merge_scan_status(per_shard):
    """The scan status of ONE tipset from its receipt-range shards' (status, phase) pairs in range order: the unsharded scan
    enumerates every receipt before it opens an events AMT, so the first shard with an Err of the RECEIPTS phase decides, and
    only when there is none the first shard with any Err (include/ipcfp.h ipcfp_witness_last_scan_phase)."""
    for st, ph in per_shard:
        if st != 1 and ph == SCAN_PHASE_RECEIPTS:
            return st
    for st, _ in per_shard:
        if st != 1:
            return st
    return 1


# event claims in transport form (include/ipcfp.h ipcfp_event_claim_compact_t / ipcfp_event_claim_group_t)
COMPACT_DTYPE = np.dtype([("emitter", np.uint64), ("exec_index", np.uint32), ("event_index", np.uint32),
                          ("message_digest", np.uint8, (32,)), ("data_len", np.uint16), ("n_topics", np.uint8),
                          ("topic_flags", np.uint8), ("flags", np.uint8), ("group", np.uint8), ("reserved", np.uint16)])
GROUP_DTYPE = np.dtype([("parent_epoch", np.int64), ("child_epoch", np.int64), ("tipset", np.uint32), ("reserved", np.uint32)])
SCLAIM_DTYPE = np.dtype([("child_epoch", np.int64), ("actor_id", np.uint64), ("child", np.uint8, (CID_SLOT,)),
                         ("state_root", np.uint8, (CID_SLOT,)), ("actor_state", np.uint8, (CID_SLOT,)),
                         ("storage_root", np.uint8, (CID_SLOT,)), ("slot", np.uint8, (32,)),
                         ("value", np.uint8, (32,)), ("flags", np.uint32), ("reserved", np.uint32)])
MATCH_DTYPE = np.dtype([("exec_index", np.uint64), ("event_index", np.uint64), ("emitter", np.uint64),
                        ("block", np.uint32), ("off", np.uint32), ("len", np.uint32), ("reserved", np.uint32)])


GEN_STORAGE_DTYPE = np.dtype([("parent_state_root", np.uint8, 40), ("actor_state_cid", np.uint8, 40),
                              ("storage_root", np.uint8, 40), ("value", np.uint8, 32), ("status", np.uint32),
                              ("reserved", np.uint32)])


STORAGE_SPEC_DTYPE = np.dtype([("actor_id", np.uint64), ("slot", np.uint8, 32)])


class EventProofSpec(C.Structure):
    """ipcfp_event_proof_spec_t == EventProofSpec (src/proofs/generator.rs:17-22)"""

    _fields_ = [("event_signature", C.c_char_p), ("topic_1", C.c_char_p), ("actor_id_filter", C.c_uint64),
                ("has_actor_id_filter", C.c_uint8)]


class EngineError(RuntimeError):
    pass


def lib_path() -> str:
    return os.environ.get("IPCFP_LIB", os.path.join(_HERE, "libipcfp.so"))


_lib = None


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load_library() -> C.CDLL:
    """Load libipcfp.so.  Raises EngineError if it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise EngineError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  This engine has no CPU fallback."
        )
    try:
        lib = C.CDLL(path)
    except OSError as e:  # pragma: no cover - depends on the box
        raise EngineError(f"cannot load {path}: {e}") from e
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    lib.ipcfp_abi_version.restype = i32
    if lib.ipcfp_abi_version() != ABI_VERSION:  # struct layouts below would be strided wrongly
        raise EngineError(f"{path} speaks ABI {lib.ipcfp_abi_version()}, this binding ABI {ABI_VERSION}: rebuild the library")
    sigs = {
        "ipcfp_abi_version": (i32, []),
        "ipcfp_strerror": (C.c_char_p, [i32]),
        "ipcfp_ctx_create": (i32, [i32, C.POINTER(vp)]),
        "ipcfp_ctx_destroy": (None, [vp]),
        "ipcfp_last_error": (C.c_char_p, [vp]),
        "ipcfp_ctx_stream": (vp, [vp]),
        "ipcfp_ctx_sync": (i32, [vp]),
        "ipcfp_ctx_set_tuning": (i32, [vp, C.c_char_p, C.c_int64]),
        "ipcfp_ctx_device_info": (i32, [vp, C.c_char_p, C.POINTER(i32), C.POINTER(u64)]),
        "ipcfp_profile_enable": (i32, [vp, i32]),
        "ipcfp_profile_reset": (i32, [vp]),
        "ipcfp_profile_read": (i32, [vp, i32, C.POINTER(u64), C.POINTER(C.c_double)]),
        "ipcfp_witness_create": (i32, [vp, vp, u64, vp, vp, vp, u64, C.POINTER(vp)]),
        "ipcfp_witness_create_packed": (i32, [vp, vp, u64, vp, vp, u64, vp, C.c_uint32, vp, vp, u64, C.POINTER(vp)]),
        "ipcfp_witness_create_device": (i32, [vp, vp, u64, vp, vp, vp, u64, C.POINTER(vp)]),
        "ipcfp_witness_destroy": (None, [vp]),
        "ipcfp_witness_block_count": (u64, [vp]),
        "ipcfp_witness_byte_count": (u64, [vp]),
        "ipcfp_witness_verify_cids": (i32, [vp, vp, vp, C.POINTER(u64)]),
        "ipcfp_witness_verify_cids_async": (i32, [vp, vp]),
        "ipcfp_witness_cid_results": (i32, [vp, vp, vp, C.POINTER(u64)]),
        "ipcfp_witness_cid_bitmap_device": (vp, [vp]),
        "ipcfp_witness_cid_status_device": (vp, [vp]),
        "ipcfp_blake2b256_batch": (i32, [vp, vp, u64, vp, vp, u64, vp]),
        "ipcfp_keccak256_batch": (i32, [vp, vp, u64, vp, vp, u64, vp]),
        "ipcfp_sha256_batch": (i32, [vp, vp, u64, vp, vp, u64, vp]),
        "ipcfp_amt_get": (i32, [vp, vp, vp, i32, i32, vp, u64, vp, vp]),
        "ipcfp_hamt_get": (i32, [vp, vp, vp, C.c_uint32, i32, vp, vp, vp, u64, vp, vp]),
        "ipcfp_hamt_get_device": (i32, [vp, vp, vp, C.c_uint32, i32, vp, vp, vp, u64, vp, vp]),
        "ipcfp_exec_order": (i32, [vp, vp, vp, C.c_uint32, vp, vp, u64, C.POINTER(u64)]),
        "ipcfp_scan_events": (i32, [vp, vp, vp, vp, i32, u64, vp, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), vp]),
        "ipcfp_verify_event_claims_device": (i32, [vp, vp, vp, C.c_uint32, vp, u64, vp, u64, vp, vp, vp]),
        "ipcfp_verify_and_scan_device": (i32, [vp, vp, vp, C.c_uint32, vp, u64, vp, u64, vp, vp, vp, vp, i32, u64, vp, vp, u64,
                                               C.POINTER(u64), vp, u64, C.POINTER(u64)]),
        "ipcfp_verify_event_claims": (i32, [vp, vp, vp, C.c_uint32, vp, u64, vp, u64, vp, vp, vp]),
        "ipcfp_compact_event_claims": (i32, [vp, u64, vp, u64, vp, C.POINTER(C.c_uint32), vp, vp, u64, C.POINTER(u64)]),
        "ipcfp_expand_event_claims_device": (i32, [vp, vp, C.c_uint32, vp, u64, vp, u64, vp, vp, u64, C.POINTER(u64)]),
        "ipcfp_verify_event_claims_compact": (i32, [vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, u64, vp, u64, vp, vp, vp]),
        "ipcfp_witness_rebuild_index": (i32, [vp, vp]),
        "ipcfp_witness_has": (i32, [vp, vp, vp, u64, vp, vp]),
        "ipcfp_witness_get": (i32, [vp, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(i32)]),
        "ipcfp_witness_put_keyed": (i32, [vp, vp, vp, vp, vp, vp, u64]),
        "ipcfp_witness_read_values": (i32, [vp, vp, vp, u64, vp, u64]),
        "ipcfp_verify_event_proofs_located": (i32, [vp, vp, vp, u64, vp, vp, vp, vp]),
        "ipcfp_verify_event_proofs_with": (i32, [vp, vp, vp, u64, vp, vp, vp, vp, vp]),
        "ipcfp_generate_proof_bundle": (i32, [vp, vp, vp, C.c_uint32, vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, u64,
                                              C.POINTER(u64), vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]),
        "ipcfp_shard_range": (None, [u64, C.c_uint32, C.c_uint32, C.POINTER(u64), C.POINTER(u64)]),
        "ipcfp_shard_plan_tipset": (i32, [vp, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, C.POINTER(u64),
                                          C.POINTER(u64), C.POINTER(u64), vp, u64, C.POINTER(u64)]),
        "ipcfp_shard_plan_tipset_all": (i32, [vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(u64), vp, vp, vp, u64,
                                              C.POINTER(u64)]),
        "ipcfp_witness_cut_host": (i32, [vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, vp, vp, vp, C.POINTER(u64)]),
        "ipcfp_route_event_claims": (i32, [vp, u64, vp, u64, u64, u64, i32, vp, vp, u64, vp, u64, C.POINTER(u64),
                                           C.POINTER(u64)]),
        "ipcfp_witness_create_subset": (i32, [vp, vp, vp, u64, u64, u64, C.POINTER(vp)]),
        "ipcfp_verify_event_claims_range": (i32, [vp, vp, vp, C.c_uint32, vp, u64, vp, u64, u64, u64, i32, vp, vp, C.POINTER(u64),
                                                  C.POINTER(u64), vp]),
        "ipcfp_witness_create_shard_pull": (i32, [vp, vp, u64, vp, vp, u64, vp, C.c_uint32, vp, vp, u64, vp, C.c_uint32, vp,
                                                  C.c_uint32, C.c_uint32, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp,
                                                  C.POINTER(vp)]),
        "ipcfp_host_register": (i32, [vp, u64]),
        "ipcfp_host_unregister": (i32, [vp]),
        "ipcfp_witness_set_receipt_range": (i32, [vp, u64, u64]),
        "ipcfp_witness_receipt_range": (None, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "ipcfp_comm_unique_id": (i32, [vp]),
        "ipcfp_comm_create": (i32, [vp, vp, i32, i32, C.POINTER(vp)]),
        "ipcfp_comm_destroy": (None, [vp]),
        "ipcfp_comm_rank": (i32, [vp]),
        "ipcfp_comm_size": (i32, [vp]),
        "ipcfp_allgather_device": (i32, [vp, vp, vp, vp, u64]),
        "ipcfp_allgather_segments": (i32, [vp, vp, vp, vp, C.c_uint32, vp, vp, u64]),
        "ipcfp_scan_events_device": (i32, [vp, vp, vp, vp, i32, u64, vp, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), vp]),
        "ipcfp_witness_last_scan_phase": (i32, [vp]),
        "ipcfp_verify_storage_claims_device": (i32, [vp, vp, vp, u64, vp, vp]),
        "ipcfp_verify_storage_claims": (i32, [vp, vp, vp, u64, vp, vp]),
        "ipcfp_compact_storage_claims": (i32, [vp, u64, C.POINTER(vp)]),
        "ipcfp_storage_columns_destroy": (None, [vp]),
        "ipcfp_storage_columns_count": (u64, [vp]),
        "ipcfp_storage_columns_runs": (vp, [vp, C.POINTER(C.c_uint32)]),
        "ipcfp_storage_columns_slots": (vp, [vp]),
        "ipcfp_storage_columns_values": (vp, [vp]),
        "ipcfp_storage_columns_cflags": (vp, [vp]),
        "ipcfp_storage_columns_bytes": (u64, [vp]),
        "ipcfp_expand_storage_claims": (i32, [vp, vp]),
        "ipcfp_verify_storage_columns_device": (i32, [vp, vp, vp, C.c_uint32, vp, vp, vp, u64, vp, vp]),
        "ipcfp_verify_storage_columns": (i32, [vp, vp, vp, vp, vp]),
        "ipcfp_expand_storage_claims_device": (i32, [vp, vp, C.c_uint32, vp, vp, vp, u64, vp]),
        "ipcfp_cid_from_string": (i32, [C.c_char_p, vp]),
        "ipcfp_cid_to_slot": (i32, [vp, C.c_uint32, vp]),
        "ipcfp_cid_to_string": (i32, [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32]),
        "ipcfp_create_event_filter": (i32, [vp, C.c_char_p, C.c_char_p, vp]),
        "ipcfp_verify_storage_proofs": (i32, [vp, vp, vp, u64, vp, vp]),
        "ipcfp_verify_event_proofs": (i32, [vp, vp, vp, u64, vp, vp, vp]),
        "ipcfp_generate_event_proofs": (i32, [vp, vp, vp, C.c_uint32, vp, vp, i32, u64, vp, vp, vp, u64, C.POINTER(u64),
                                              vp, vp, u64, C.POINTER(u64)]),
        "ipcfp_generate_storage_proofs": (i32, [vp, vp, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64)]),
        "ipcfp_pack_event_proofs": (i32, [vp, u64, C.POINTER(vp)]),
        "ipcfp_pack_storage_proofs": (i32, [vp, u64, vp]),
        "ipcfp_packed_events_destroy": (None, [vp]),
        "ipcfp_packed_events_tipsets": (vp, [vp, C.POINTER(C.c_uint32)]),
        "ipcfp_packed_events_claims": (vp, [vp, C.POINTER(u64)]),
        "ipcfp_packed_events_blob": (vp, [vp, C.POINTER(u64)]),
        "ipcfp_bundle_parse_json": (i32, [vp, C.c_char_p, u64, C.c_uint32, C.POINTER(vp)]),
        "ipcfp_bundle_destroy": (None, [vp]),
        "ipcfp_bundle_check_json": (i32, [C.c_char_p, u64, C.c_uint32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64),
                                          C.c_char_p, C.c_uint32]),
        "ipcfp_bundle_witness": (vp, [vp]),
        "ipcfp_bundle_block_count": (u64, [vp]),
        "ipcfp_bundle_event_count": (u64, [vp]),
        "ipcfp_bundle_storage_count": (u64, [vp]),
        "ipcfp_bundle_event_proofs": (vp, [vp]),
        "ipcfp_bundle_storage_proofs": (vp, [vp]),
        "ipcfp_verify_proof_bundle": (i32, [vp, vp, vp, vp, vp, vp]),
        "ipcfp_event_claims_from_matches_device": (i32, [vp, vp, vp, u64, vp, C.c_int64, C.c_int64, C.c_uint32, vp, vp, u64, C.POINTER(u64)]),
        "ipcfp_generate_event_claims": (i32, [vp, vp, vp, C.c_uint32, vp, vp, i32, u64, vp, C.POINTER(vp)]),
        "ipcfp_generate_event_claims_tipsets": (i32, [vp, vp, vp, vp, vp, C.c_uint32, vp, i32, u64, C.POINTER(vp)]),
        "ipcfp_generated_events_tipset_count": (C.c_uint32, [vp]),
        "ipcfp_generated_events_tipsets": (vp, [vp, C.POINTER(C.c_uint32)]),
        "ipcfp_generated_events_tipset_status": (vp, [vp, C.POINTER(C.c_uint32)]),
        "ipcfp_generated_events_tipset_claim_off": (vp, [vp, C.POINTER(C.c_uint32)]),
        "ipcfp_generated_events_destroy": (None, [vp]),
        "ipcfp_generated_events_count": (u64, [vp]),
        "ipcfp_generated_events_tipset": (vp, [vp]),
        "ipcfp_generated_events_claims_device": (vp, [vp]),
        "ipcfp_generated_events_blob_device": (vp, [vp, C.POINTER(u64)]),
        "ipcfp_generated_events_copy": (i32, [vp, vp, vp, u64]),
        "ipcfp_generated_events_matches": (vp, [vp, C.POINTER(u64)]),
        "ipcfp_generated_events_message_cids": (vp, [vp, C.POINTER(u64)]),
        "ipcfp_generated_events_block_ids": (vp, [vp, C.POINTER(u64)]),
        "ipcfp_generated_events_proofs": (i32, [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]),
        "ipcfp_unpack_event_claims": (i32, [vp, C.c_uint32, vp, u64, vp, u64, C.POINTER(vp), C.POINTER(u64)]),
        "ipcfp_unpacked_events_proofs": (vp, [vp, C.POINTER(u64)]),
        "ipcfp_unpacked_events_destroy": (None, [vp]),
        "ipcfp_generate_storage_claims": (i32, [vp, vp, vp, C.c_int64, vp, vp, u64, C.POINTER(vp)]),
        "ipcfp_generate_storage_claims_device": (i32, [vp, vp, vp, C.c_int64, vp, vp, u64, C.POINTER(vp)]),
        "ipcfp_generate_storage_claims_tipsets": (i32, [vp, vp, vp, vp, C.c_uint32, vp, vp, u64, C.POINTER(vp)]),
        "ipcfp_generate_storage_claims_tipsets_device": (i32, [vp, vp, vp, vp, C.c_uint32, vp, vp, u64, C.POINTER(vp)]),
        "ipcfp_generated_storage_claims_tipset_count": (C.c_uint32, [vp]),
        "ipcfp_generated_storage_claims_tipset_first_error": (u64, [vp, C.c_uint32]),
        "ipcfp_generated_storage_claims_tipset_block_ids": (vp, [vp, C.c_uint32, C.POINTER(u64)]),
        "ipcfp_generated_storage_claims_destroy": (None, [vp]),
        "ipcfp_generated_storage_claims_count": (u64, [vp]),
        "ipcfp_generated_storage_claims_run_count": (C.c_uint32, [vp]),
        "ipcfp_generated_storage_claims_runs_device": (vp, [vp]),
        "ipcfp_generated_storage_claims_slots_device": (vp, [vp]),
        "ipcfp_generated_storage_claims_values_device": (vp, [vp]),
        "ipcfp_generated_storage_claims_cflags_device": (vp, [vp]),
        "ipcfp_generated_storage_claims_status_device": (vp, [vp]),
        "ipcfp_generated_storage_claims_status": (vp, [vp, C.POINTER(u64)]),
        "ipcfp_generated_storage_claims_first_error": (u64, [vp]),
        "ipcfp_generated_storage_claims_copy": (i32, [vp, vp, vp, vp, vp]),
        "ipcfp_generated_storage_claims_block_ids": (vp, [vp, C.POINTER(u64)]),
        "ipcfp_generated_storage_claims_proofs": (i32, [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]),
        "ipcfp_unpack_storage_claims": (i32, [vp, u64, C.POINTER(vp), C.POINTER(u64)]),
        "ipcfp_unpacked_storage_proofs": (vp, [vp, C.POINTER(u64)]),
        "ipcfp_unpacked_storage_destroy": (None, [vp]),
        "ipcfp_bundle_write_claims_json": (i32, [vp, u64, vp, u64, vp, u64, C.POINTER(u64)]),
        "ipcfp_bundle_write_json": (i32, [vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, C.POINTER(u64)]),
        "ipcfp_bundle_write_packed_json": (i32, [vp, vp, vp, C.c_uint32, vp, vp, vp, u64, vp, C.c_uint32, vp, u64, vp, u64, vp, u64,
                                                 vp, u64, C.POINTER(u64), C.POINTER(C.c_int), C.POINTER(u64)]),
        "ipcfp_bundle_write_generated_json": (i32, [vp, vp, vp, vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(C.c_int),
                                                    C.POINTER(u64)]),
        "ipcfp_scan_events_multi": (i32, [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, u64, C.POINTER(u64), vp, vp, u64, C.POINTER(u64), vp, vp]),
        "ipcfp_scan_events_multi_device": (i32, [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, u64, C.POINTER(u64), vp, vp, u64, C.POINTER(u64), vp, vp]),
        "ipcfp_scan_events_tipsets": (i32, [vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp, u64, C.POINTER(u64), vp, vp, u64, C.POINTER(u64), vp, vp]),
        "ipcfp_scan_events_tipsets_device": (i32, [vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64), vp, vp, u64, C.POINTER(u64), vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _table(blocks):
    """list[bytes] → (bytes u8[], off u64[], len u32[]) packed back to back."""
    lens = np.fromiter((len(b) for b in blocks), dtype=np.uint32, count=len(blocks))
    off = np.zeros(len(blocks), dtype=np.uint64)
    if len(blocks):
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = np.frombuffer(b"".join(blocks), dtype=np.uint8).copy() if len(blocks) else np.zeros(0, np.uint8)
    return data, off, lens


class Engine:
    """One GPU context (``ipcfp_ctx_t``)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.ipcfp_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise EngineError(f"ipcfp_ctx_create(device={device}) failed: {self.lib.ipcfp_strerror(rc).decode()}")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.ipcfp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- helpers ---------------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.ipcfp_last_error(self.h).decode(errors="replace")
            raise EngineError(f"{what}: {self.lib.ipcfp_strerror(rc).decode()} ({rc}) {msg}")

    def set_tuning(self, key: str, value: int):
        """Route selection (ipcfp_ctx_set_tuning): "hamt_levels", "hamt_table", "fast_verify"; the side grids'
        workgroups per CU, "k1_resident" and "parse_resident" (0..16)."""
        self._check(self.lib.ipcfp_ctx_set_tuning(self.h, key.encode(), int(value)), "ctx_set_tuning")

    def sync(self):
        self._check(self.lib.ipcfp_ctx_sync(self.h), "sync")

    @property
    def stream_ptr(self) -> int:
        return int(self.lib.ipcfp_ctx_stream(self.h) or 0)

    def device_info(self):
        name = C.create_string_buffer(64)
        cus = C.c_int()
        mem = C.c_uint64()
        self._check(self.lib.ipcfp_ctx_device_info(self.h, name, C.byref(cus), C.byref(mem)), "device_info")
        return {"name": name.value.decode(), "cus": cus.value, "hbm_bytes": mem.value}

    # -- profiling ---------------------------------------------------------------
    def profile_enable(self, on: bool = True, only: str | None = None):
        """`only`: bracket the launches of that kernel id alone (the others stay back to back on the stream)."""
        self._check(self.lib.ipcfp_profile_enable(self.h, (2 + KERNEL_IDS[only]) if (on and only) else (1 if on else 0)), "profile_enable")

    def profile_reset(self):
        self._check(self.lib.ipcfp_profile_reset(self.h), "profile_reset")

    def profile_read(self, kernel: str):
        n = C.c_uint64()
        ms = C.c_double()
        self._check(self.lib.ipcfp_profile_read(self.h, KERNEL_IDS[kernel], C.byref(n), C.byref(ms)), "profile_read")
        return n.value, ms.value

    # -- a bundle's JSON text from packed claims resident in HBM ---------------------------------
    def _bundle_write_packed(self, what, call, cap):
        """The two-call buffer contract around `call(out, cap, len, bad_kind, bad_index)`.  cap None: sizing call, then
        a buffer of exactly that size → the text; an int: ONE call with that capacity → (rc, len, buffer).
        A refusal raises EngineError with `.rc`, `.bad_kind` (0 storage, 1 events, 2 blocks) and `.bad_index` (None: no index)."""
        n, kind, bad = C.c_uint64(), C.c_int(), C.c_uint64()

        def check(rc):
            if rc != 0:
                msg = self.lib.ipcfp_last_error(self.h)
                e = EngineError(f"{what}: {msg.decode() if msg else ''} ({rc})")
                e.rc, e.bad_kind, e.bad_index = rc, int(kind.value), (None if bad.value == 2**64 - 1 else int(bad.value))
                raise e

        if cap is not None:
            out = np.full(max(int(cap), 1), 0xA5, dtype=np.uint8)
            rc = call(_p(out) if cap else None, int(cap), C.byref(n), C.byref(kind), C.byref(bad))
            return int(rc), int(n.value), out[: int(cap)]
        check(call(None, 0, C.byref(n), C.byref(kind), C.byref(bad)))
        out = np.empty(max(int(n.value), 1), dtype=np.uint8)
        check(call(_p(out), int(n.value), C.byref(n), C.byref(kind), C.byref(bad)))
        return out[: int(n.value)].tobytes()

    def bundle_write_packed_json(self, witness, runs_ptr: int, n_runs: int, slot_ptr: int, value_ptr: int, cflags_ptr: int,
                                 n_storage: int, tipsets, claims_ptr: int, n_events: int, blob_ptr: int, blob_len: int,
                                 block_ids=None, cap=None):
        """`serde_json::to_string(&UnifiedProofBundle)` of packed claims resident in HBM (ipcfp_bundle_write_packed_json): the
        storage claims in column form and the event claims + blob as DEVICE addresses, `tipsets` a host TIPSET_DTYPE array,
        the listed blocks of `witness` (None: every block in id order).  The claims head is written on the device."""
        ts = np.ascontiguousarray(tipsets, dtype=TIPSET_DTYPE) if tipsets is not None else np.zeros(0, dtype=TIPSET_DTYPE)
        if block_ids is None:
            ids, nb = None, witness.n
        else:
            ids = np.ascontiguousarray(block_ids, dtype=np.uint32)
            nb = len(ids)

        def call(out, cap_, n, kind, bad):
            return self.lib.ipcfp_bundle_write_packed_json(
                self.h, witness.h, runs_ptr or None, int(n_runs), slot_ptr or None, value_ptr or None, cflags_ptr or None,
                int(n_storage), _p(ts) if len(ts) else None, len(ts), claims_ptr or None, int(n_events), blob_ptr or None,
                int(blob_len), _p(ids), nb, out, cap_, n, kind, bad)

        return self._bundle_write_packed("bundle_write_packed_json", call, cap)

    def bundle_write_generated_json(self, witness, gs, ge, block_ids=None, cap=None):
        """The same fed from the generators' handles (GeneratedStorageClaims / GeneratedEvents; None: an empty list):
        ipcfp_bundle_write_generated_json."""
        if block_ids is None:
            ids, nb = None, witness.n
        else:
            ids = np.ascontiguousarray(block_ids, dtype=np.uint32)
            nb = len(ids)

        def call(out, cap_, n, kind, bad):
            return self.lib.ipcfp_bundle_write_generated_json(self.h, witness.h, gs.h if gs is not None else None,
                                                              ge.h if ge is not None else None, _p(ids), nb, out, cap_, n, kind, bad)

        return self._bundle_write_packed("bundle_write_generated_json", call, cap)

    # -- batch hashes ------------------------------------------------------------
    def _hash(self, fn, data, off, lens):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = len(off)
        out = np.zeros((n, 32), dtype=np.uint8)
        self._check(fn(self.h, _p(data), data.size, _p(off), _p(lens), n, _p(out)), fn.__name__)
        return out

    def blake2b256(self, data, off, lens):
        return self._hash(self.lib.ipcfp_blake2b256_batch, data, off, lens)

    def keccak256(self, data, off, lens):
        return self._hash(self.lib.ipcfp_keccak256_batch, data, off, lens)

    def sha256(self, data, off, lens):
        return self._hash(self.lib.ipcfp_sha256_batch, data, off, lens)

    def blake2b256_list(self, msgs):
        return self.blake2b256(*_table(msgs))

    def keccak256_list(self, msgs):
        return self.keccak256(*_table(msgs))

    def sha256_list(self, msgs):
        return self.sha256(*_table(msgs))

    def create_event_filter(self, event_sig: str, subnet_id: str):
        """(topic0, topic1) of create_event_filter; topic0 is hashed on the device."""
        out = np.zeros(64, dtype=np.uint8)
        self._check(self.lib.ipcfp_create_event_filter(self.h, event_sig.encode(), subnet_id.encode(), _p(out)),
                    "create_event_filter")
        return out[:32].tobytes(), out[32:].tobytes()

    # -- witness -------------------------------------------------------------------
    def witness(self, data, off, lens, cids40) -> "Witness":
        return Witness(self, data, off, lens, cids40)

    def bundle(self, text: bytes, flags: int = 0) -> "Bundle":
        """Parse a `UnifiedProofBundle` JSON; the blocks are base64-decoded on the device."""
        return Bundle(self, text, flags)

    def witness_from_blocks(self, blocks, cids) -> "Witness":
        """blocks: list[bytes]; cids: list[bytes] binary CIDs (≤ 40 B each)."""
        data, off, lens = _table(blocks)
        return Witness(self, data, off, lens, pack_cids(cids))

    def expand_event_claims_device(self, groups: np.ndarray, compact_ptr: int, n: int, cblob_ptr: int, cblob_len: int,
                                   claims_out_ptr: int, blob_out_ptr: int, cap_blob: int) -> int:
        """Transport form → ipcfp_event_claim_t[n] + blob, all resident in HBM; returns the blob's length."""
        groups = np.ascontiguousarray(groups, dtype=GROUP_DTYPE)
        bl = C.c_uint64()
        self._check(self.lib.ipcfp_expand_event_claims_device(self.h, _p(groups), len(groups), compact_ptr, n, cblob_ptr, cblob_len,
                                                              claims_out_ptr, blob_out_ptr, cap_blob, C.byref(bl)), "expand_event_claims")
        return int(bl.value)

    def witness_packed(self, packed: "PackedWitnessTables") -> "Witness":
        """The witness from its tables in transport form (ipcfp_witness_create_packed): no offset table, 32-byte digests."""
        return Witness(self, None, None, None, None, packed=packed)

    def witness_shard_pull(self, packed: "PackedWitnessTables", parent_cids, child_cid: bytes, n_shards: int, shard: int):
        """Rank `shard` of `n_shards` pulls its receipt-range shard of one tipset out of the bundle `packed` in host memory
        (ipcfp_witness_create_shard_pull; packed.data must be device-readable: `host_register(packed.data)` or pinned).
        Returns (status, Witness | None, receipt_lo, receipt_hi, n_receipts, stats dict)."""
        pk = packed
        pc = pack_cids(parent_cids)
        child = cid_slots([child_cid])[0].copy()
        st = np.zeros(1, dtype=np.uint8)
        lo, hi, nr = C.c_uint64(), C.c_uint64(), C.c_uint64()
        stats = ShardPullStats()
        h = C.c_void_p()
        self._check(self.lib.ipcfp_witness_create_shard_pull(
            self.h, _p(pk.data), pk.data.size, _p(pk.lens), _p(pk.digests), len(pk.lens), _p(pk.prefix), len(pk.prefix),
            _p(pk.esc_index), _p(pk.esc_cids), len(pk.esc_index), _p(pc), len(parent_cids), _p(child), int(n_shards), int(shard),
            _p(st), C.byref(lo), C.byref(hi), C.byref(nr), C.cast(C.pointer(stats), C.c_void_p), C.byref(h)), "witness_create_shard_pull")
        w = None
        if h.value:
            w = Witness.__new__(Witness)
            w.eng, w.lib, w.h, w.n = self, self.lib, h, int(stats.blocks)
        sd = {f: getattr(stats, f) for f, _ in ShardPullStats._fields_}
        return int(st[0]), w, int(lo.value), int(hi.value), int(nr.value), sd

    def witness_device(self, bytes_ptr, nbytes, off_ptr, len_ptr, cids_ptr, n) -> "Witness":
        return Witness(self, None, None, None, None, device=(bytes_ptr, nbytes, off_ptr, len_ptr, cids_ptr, n))


class ShardPullStats(C.Structure):  # == ipcfp_shard_pull_stats_t
    _fields_ = [("rounds", C.c_uint32), ("blocks", C.c_uint32), ("table_bytes", C.c_uint64), ("block_bytes", C.c_uint64),
                ("payload_bytes", C.c_uint64), ("tables_ms", C.c_double), ("pull_ms", C.c_double), ("create_ms", C.c_double)]


PAGE = 4096


def ingest_buffer(nbytes: int) -> np.ndarray:
    """A host byte buffer that OWNS its pages (an anonymous mapping: page-aligned, whole pages) — what an ingest buffer
    handed to `host_register` has to be.  The array keeps the mapping alive."""
    import mmap

    # (private: a shared anonymous mapping is shmem-backed, which userptr registration may refuse)
    m = mmap.mmap(-1, max((int(nbytes) + PAGE - 1) // PAGE * PAGE, PAGE), flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
    return np.frombuffer(m, dtype=np.uint8)[: int(nbytes)]


def host_register(arr: np.ndarray):
    """Map a host array for device reads (ipcfp_host_register = hipHostRegister): what ipcfp_witness_create_shard_pull's
    `bytes` must be.  An ingest buffer is registered once, when it is made — and it must own its pages (`ingest_buffer`,
    `PackedWitnessTables(..., ingest=True)`): registration is by page, and a page shared with other host memory (a heap
    allocation, or an array the runtime has also pinned as the pageable source of a copy) loses its device mapping for
    that other user when this one is unregistered — a GPU memory fault in a later, unrelated copy."""
    if arr.ctypes.data % PAGE:
        raise EngineError("host_register: the buffer does not start on a page boundary (use ingest_buffer / PackedWitnessTables(..., ingest=True))")
    rc = load_library().ipcfp_host_register(_p(arr), arr.nbytes)
    if rc:
        raise EngineError(f"host_register: {load_library().ipcfp_strerror(rc).decode()}")


def host_unregister(arr: np.ndarray):
    rc = load_library().ipcfp_host_unregister(_p(arr))
    if rc:
        raise EngineError(f"host_unregister: {load_library().ipcfp_strerror(rc).decode()}")


STD_CID_PREFIX = bytes.fromhex("0171a0e40220")  # CIDv1, dag-cbor, blake2b-256, 32-byte digest


class PackedWitnessTables:
    """A witness's tables in the transport form of ipcfp_witness_create_packed: the blocks back to back (no offset
    table), one 32-byte digest per block + the CID prefix they share, and the blocks whose CID has another form as
    (index, 40-byte slot) escapes.  `h2d_bytes` is what crosses PCIe."""

    def __init__(self, data, off, lens, cids40, prefix: bytes = STD_CID_PREFIX, ingest: bool = False):
        """ingest=True: `data` and `digests` are copied into buffers that own their pages (`ingest_buffer`), fit for
        `host_register` — the form a rank's ingest path would receive a bundle in."""
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        cids40 = np.ascontiguousarray(cids40, dtype=np.uint8).reshape(-1, CID_SLOT)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        n = len(lens)
        tight = np.zeros(n, dtype=np.uint64)
        if n:
            tight[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        if n and not (np.array_equal(tight, off) and int(tight[-1]) + int(lens[-1]) == data.size):
            # the caller's blocks are not back to back: lay them out so (a host copy; a bundle's blocks arrive one by one anyway)
            out = np.empty(int(lens.sum(dtype=np.uint64)), dtype=np.uint8)
            for i in range(n):
                out[int(tight[i]): int(tight[i]) + int(lens[i])] = data[int(off[i]): int(off[i]) + int(lens[i])]
            data = out
        self.data, self.lens = data, lens
        pl = len(prefix)
        self.prefix = np.frombuffer(bytes(prefix), dtype=np.uint8).copy()
        std = np.ones(n, dtype=bool)
        if n:
            std &= (cids40[:, :pl] == self.prefix[None, :]).all(axis=1)
            std &= (cids40[:, pl + 32:] == 0).all(axis=1)
        self.digests = np.ascontiguousarray(cids40[:, pl: pl + 32])
        if ingest:
            own = ingest_buffer(self.data.size)
            own[:] = self.data
            self.data = own
            own = ingest_buffer(self.digests.size).reshape(-1, 32)
            own[:] = self.digests
            self.digests = own
        self.esc_index = np.ascontiguousarray(np.nonzero(~std)[0].astype(np.uint32))
        self.esc_cids = np.ascontiguousarray(cids40[~std])
        self.h2d_bytes = int(self.data.size + self.lens.nbytes + self.digests.nbytes + self.esc_index.nbytes + self.esc_cids.nbytes)


def shard_range(n: int, n_shards: int, shard: int):
    """[lo, hi) of `shard` when n units are cut into n_shards contiguous ranges (host only, no GPU)."""
    lo, hi = C.c_uint64(), C.c_uint64()
    load_library().ipcfp_shard_range(int(n), int(n_shards), int(shard), C.byref(lo), C.byref(hi))
    return int(lo.value), int(hi.value)


def witness_cut_host(data, off, lens, cids40, block_ids):
    """Host only: blocks `block_ids` of a host-resident witness as a packed witness of their own
    → (data u8[], off u64[], lens u32[], cids u8[n, 40])."""
    lib = load_library()
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    cids40 = np.ascontiguousarray(cids40, dtype=np.uint8)
    ids = np.ascontiguousarray(block_ids, dtype=np.uint32)
    nb = C.c_uint64()
    rc = lib.ipcfp_witness_cut_host(_p(data), data.size, _p(off), _p(lens), _p(cids40), len(lens), _p(ids), len(ids),
                                    None, 0, None, None, None, C.byref(nb))
    if rc:
        raise EngineError(f"witness_cut_host: {lib.ipcfp_strerror(rc).decode()}")
    out = np.empty(int(nb.value), dtype=np.uint8)
    o_off = np.empty(len(ids), dtype=np.uint64)
    o_len = np.empty(len(ids), dtype=np.uint32)
    o_cids = np.empty((len(ids), CID_SLOT), dtype=np.uint8)
    rc = lib.ipcfp_witness_cut_host(_p(data), data.size, _p(off), _p(lens), _p(cids40), len(lens), _p(ids), len(ids),
                                    _p(out), out.size, _p(o_off), _p(o_len), _p(o_cids), C.byref(nb))
    if rc:
        raise EngineError(f"witness_cut_host: {lib.ipcfp_strerror(rc).decode()}")
    return out, o_off, o_len, o_cids


def route_event_claims(claims: np.ndarray, blob: np.ndarray, blob_len: int, lo: int, hi: int, last: bool):
    """Host only: the packed claims of the receipt-range shard [lo, hi) (ipcfp_route_event_claims)
    → (positions u64[], claims, blob u8[] + 64 B slack, blob_len)."""
    lib = load_library()
    claims = np.ascontiguousarray(claims)
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n_out, b_out = C.c_uint64(), C.c_uint64()
    args = (_p(claims), len(claims), _p(blob), int(blob_len), int(lo), int(hi), int(bool(last)))
    rc = lib.ipcfp_route_event_claims(*args, None, None, 0, None, 0, C.byref(n_out), C.byref(b_out))
    if rc:
        raise EngineError(f"route_event_claims: {lib.ipcfp_strerror(rc).decode()}")
    n, nb = int(n_out.value), int(b_out.value)
    pos = np.empty(n, dtype=np.uint64)
    out = np.zeros(n, dtype=CLAIM_DTYPE)
    oblob = np.zeros(nb + 64, dtype=np.uint8)
    rc = lib.ipcfp_route_event_claims(*args, _p(pos), _p(out), n, _p(oblob), nb, C.byref(n_out), C.byref(b_out))
    if rc:
        raise EngineError(f"route_event_claims: {lib.ipcfp_strerror(rc).decode()}")
    return pos, out, oblob, nb


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the engine's run-time binding of librccl (rank 0 calls this; the host carries
    the 128 bytes to the other ranks)."""
    lib = load_library()
    buf = np.zeros(128, dtype=np.uint8)
    rc = lib.ipcfp_comm_unique_id(_p(buf))
    if rc != 0:
        raise EngineError(f"comm_unique_id: {lib.ipcfp_strerror(rc).decode()} ({rc})")
    return buf.tobytes()


class Comm:
    """One rank of an RCCL communicator (``ipcfp_comm_t``) bound to an Engine's GPU and stream."""

    def __init__(self, eng: "Engine", unique_id: bytes, n_ranks: int, rank: int):
        self.eng = eng
        self.lib = eng.lib
        h = C.c_void_p()
        idb = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
        eng._check(self.lib.ipcfp_comm_create(eng.h, _p(idb), int(n_ranks), int(rank), C.byref(h)), "comm_create")
        self.h = h
        self.n_ranks, self.rank = int(n_ranks), int(rank)

    def allgather_device(self, send_ptr: int, recv_ptr: int, bytes_per_rank: int):
        """ncclAllGather of bytes_per_rank bytes per rank on the engine's stream (asynchronous)."""
        self.eng._check(self.lib.ipcfp_allgather_device(self.eng.h, self.h, send_ptr, recv_ptr, int(bytes_per_rank)),
                        "allgather_device")

    def allgather_segments(self, seg_ptrs, seg_bytes, staging_ptr: int, recv_ptr: int, bytes_per_rank: int):
        allgather_segments(self.eng, self, seg_ptrs, seg_bytes, staging_ptr, recv_ptr, bytes_per_rank)

    def close(self):
        if getattr(self, "h", None):
            if self.eng.h:
                self.lib.ipcfp_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def allgather_segments(eng: "Engine", comm, seg_ptrs, seg_bytes, staging_ptr: int, recv_ptr: int, bytes_per_rank: int):
    """Pack the device segments back to back into staging (zero padded to bytes_per_rank) and all-gather them —
    one collective; comm=None: a single rank, the packed message is the result."""
    n = len(seg_ptrs)
    ptrs = (C.c_void_p * max(n, 1))(*[int(p) for p in seg_ptrs])
    lens = (C.c_uint64 * max(n, 1))(*[int(b) for b in seg_bytes])
    eng._check(eng.lib.ipcfp_allgather_segments(eng.h, comm.h if comm is not None else None,
                                                C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n, staging_ptr,
                                                recv_ptr, int(bytes_per_rank)), "allgather_segments")


def pack_event_claims(parent_cids, child_cid, parent_epoch, child_epoch, exec_index, event_index, emitter,
                      message_cids40, n_topics, topics, data_len, data):
    """Lower binary event claims of ONE tipset to the packed ABI form (ipcfp_tipset_ref_t[1],
    ipcfp_event_claim_t[n], blob).  topics: u8[n, 4, 32]; data: u8[n, dmax].  All flags are set: binary
    inputs correspond to strings that parsed."""
    n = len(exec_index)
    ts = np.zeros(1, dtype=TIPSET_DTYPE).view(TipsetRefs)
    ts["flags"] = 3
    ts["n_parents"] = len(parent_cids)
    ts["child"][0] = cid_slots([child_cid])[0]
    slots = cid_slots(parent_cids)
    ts["parents"][0, : min(len(slots), MAX_PARENTS)] = slots[:MAX_PARENTS]
    if len(slots) > MAX_PARENTS:  # a tipset key wider than the inline form: the rest behind `more_parents`
        more = np.ascontiguousarray(slots[MAX_PARENTS:])
        ts._keep = [more]
        ts["more_parents"] = more.ctypes.data
    cl = np.zeros(n, dtype=CLAIM_DTYPE)
    cl["parent_epoch"] = parent_epoch
    cl["child_epoch"] = child_epoch
    cl["exec_index"] = exec_index
    cl["event_index"] = event_index
    cl["emitter"] = emitter
    cl["message_cid"] = message_cids40
    cl["flags"] = 3
    cl["n_topics"] = n_topics
    # blob: per claim n_topics × [1, topic(32)] then data
    nt = np.asarray(n_topics, dtype=np.int64)
    dl = np.asarray(data_len, dtype=np.int64)
    sizes = nt * 33 + dl
    starts = np.zeros(n, dtype=np.int64)
    if n:
        starts[1:] = np.cumsum(sizes[:-1])
    total = int(sizes.sum())
    blob = np.zeros(total + 64, dtype=np.uint8)
    cl["topics_off"] = starts
    cl["data_off"] = starts + nt * 33
    cl["data_len"] = dl
    for t in range(topics.shape[1]):
        sel = np.nonzero(nt > t)[0]
        if len(sel) == 0:
            continue
        base = starts[sel] + 33 * t
        blob[base] = 1
        idx = base[:, None] + 1 + np.arange(32)[None, :]
        blob[idx] = topics[sel, t]
    dmax = data.shape[1]
    for j in range(dmax):
        sel = np.nonzero(dl > j)[0]
        if len(sel) == 0:
            break
        blob[starts[sel] + nt[sel] * 33 + j] = data[sel, j]
    return ts, cl, blob[: total + 64], total


def compact_event_claims(claims: np.ndarray, blob: np.ndarray, blob_len: int):
    """Packed claims → transport form (ipcfp_compact_event_claims, host only): (groups, compact records, blob, blob_len).
    Raises EngineError when the batch is not representable (the caller keeps the plain form)."""
    claims = np.ascontiguousarray(claims, dtype=CLAIM_DTYPE)
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n = len(claims)
    groups = np.zeros(256, dtype=GROUP_DTYPE)
    out = np.zeros(n, dtype=COMPACT_DTYPE)
    out_blob = np.zeros(int(blob_len) + 64, dtype=np.uint8)
    ng, ol = C.c_uint32(), C.c_uint64()
    rc = load_library().ipcfp_compact_event_claims(_p(claims), n, _p(blob), int(blob_len), _p(groups), C.byref(ng), _p(out),
                                                   _p(out_blob), int(blob_len), C.byref(ol))
    if rc:
        raise EngineError(f"compact_event_claims: not representable in transport form ({rc})")
    return groups[: ng.value].copy(), out, out_blob, int(ol.value)


def pack_storage_claims(child_cid, state_root, child_epoch, actor_id, actor_state40, storage_root40, slot32, value32):
    """Binary storage claims → ipcfp_storage_claim_t[n] with every flag set."""
    n = len(actor_id)
    cl = np.zeros(n, dtype=SCLAIM_DTYPE)
    cl["child_epoch"] = child_epoch
    cl["actor_id"] = actor_id
    cl["child"][:] = cid_slots([child_cid])[0]
    cl["state_root"][:] = cid_slots([state_root])[0]
    cl["actor_state"] = actor_state40
    cl["storage_root"] = storage_root40
    cl["slot"] = slot32
    cl["value"] = value32
    cl["flags"] = 63
    return cl


def cid_from_string(s: str):
    """Host-side `Cid::try_from(&str)` of the engine: bytes, or None where the reference returns Err."""
    out = np.zeros(CID_SLOT, dtype=np.uint8)
    n = load_library().ipcfp_cid_from_string(s.encode(), _p(out))
    return out.tobytes()[:n] if n > 0 else None


def cid_to_string(cid: bytes):
    buf = C.create_string_buffer(256)
    n = load_library().ipcfp_cid_to_string(bytes(cid), len(cid), buf, 256)
    return buf.value.decode() if n > 0 else None


def pack_cids(cids) -> np.ndarray:
    """[binary CID, …] → u8[n, 40]: zero padded; a CID longer than the slot folded (cid_slot)."""
    return cid_slots(cids)


def pack_event_proofs(claims_arr, n: int):
    """Host-only lowering of an array of ipcfp_event_proof_t (strings) to the packed ABI form (no GPU):
    → (tipsets TIPSET_DTYPE[], claims CLAIM_DTYPE[n], blob u8[])."""
    lib = load_library()
    h = C.c_void_p()
    rc = lib.ipcfp_pack_event_proofs(C.cast(claims_arr, C.c_void_p), n, C.byref(h))
    if rc != 0:
        raise EngineError(f"pack_event_proofs: {lib.ipcfp_strerror(rc).decode()} ({rc})")
    try:
        nt, nc, nb = C.c_uint32(), C.c_uint64(), C.c_uint64()
        pt = lib.ipcfp_packed_events_tipsets(h, C.byref(nt))
        pc = lib.ipcfp_packed_events_claims(h, C.byref(nc))
        pb = lib.ipcfp_packed_events_blob(h, C.byref(nb))

        def view(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype=dtype)
            buf = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype).copy()

        ts = view(pt, nt.value, TIPSET_DTYPE).view(TipsetRefs)
        ts._keep = []
        for k in range(len(ts)):  # a key wider than the inline form: its tail is the handle's — copied before the handle goes
            extra = int(ts["n_parents"][k]) - MAX_PARENTS
            if extra > 0:
                more = view(int(ts["more_parents"][k]), extra * CID_SLOT, np.uint8)
                ts._keep.append(more)
                ts["more_parents"][k] = more.ctypes.data
        return ts, view(pc, nc.value, CLAIM_DTYPE), view(pb, nb.value, np.uint8)
    finally:
        lib.ipcfp_packed_events_destroy(h)


def pack_storage_proofs(claims_arr, n: int) -> np.ndarray:
    """Host-only lowering of an array of ipcfp_storage_proof_t (strings) → SCLAIM_DTYPE[n] (no GPU)."""
    lib = load_library()
    out = np.zeros(n, dtype=SCLAIM_DTYPE)
    rc = lib.ipcfp_pack_storage_proofs(C.cast(claims_arr, C.c_void_p), n, _p(out))
    if rc != 0:
        raise EngineError(f"pack_storage_proofs: {lib.ipcfp_strerror(rc).decode()} ({rc})")
    return out


# one record of the run table of the column form (include/ipcfp.h IPCFP_SRUN_*; private to the binding)
_SRUN_DTYPE = np.dtype([("child_epoch", np.int64), ("actor_id", np.uint64), ("child", np.uint8, (CID_SLOT,)),
                        ("state_root", np.uint8, (CID_SLOT,)), ("actor_state", np.uint8, (CID_SLOT,)),
                        ("storage_root", np.uint8, (CID_SLOT,)), ("first_claim", np.uint32), ("n_claims", np.uint32),
                        ("flags", np.uint32), ("reserved", np.uint32)])
assert _SRUN_DTYPE.itemsize == 192


class StorageColumns:
    """Storage claims in run-compressed, column form (ipcfp_storage_columns_t): owns the handle; `runs`, `slot`, `value`,
    `cflags` are numpy views of the handle's memory (valid until close())."""

    def __init__(self, handle):
        self.lib = load_library()
        self.h = handle
        lib = self.lib
        self.n = int(lib.ipcfp_storage_columns_count(handle))
        nr = C.c_uint32()
        pr = lib.ipcfp_storage_columns_runs(handle, C.byref(nr))
        self.n_runs = int(nr.value)
        self.nbytes = int(lib.ipcfp_storage_columns_bytes(handle))

        def view(ptr, count, dtype, shape):
            if not count:
                return np.zeros(shape, dtype=dtype)
            buf = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype).reshape(shape)

        self.runs = view(pr, self.n_runs, _SRUN_DTYPE, (self.n_runs,))
        self.slot = view(lib.ipcfp_storage_columns_slots(handle), self.n * 32, np.uint8, (self.n, 32))
        self.value = view(lib.ipcfp_storage_columns_values(handle), self.n * 32, np.uint8, (self.n, 32))
        self.cflags = view(lib.ipcfp_storage_columns_cflags(handle), self.n, np.uint8, (self.n,))

    def close(self):
        if self.h:
            self.runs = self.slot = self.value = self.cflags = None
            self.lib.ipcfp_storage_columns_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def compact_storage_claims(claims: np.ndarray) -> StorageColumns:
    """Host-only: SCLAIM_DTYPE[n] → the column form with maximal runs (ipcfp_compact_storage_claims; no GPU)."""
    lib = load_library()
    claims = np.ascontiguousarray(claims, dtype=SCLAIM_DTYPE)
    h = C.c_void_p()
    rc = lib.ipcfp_compact_storage_claims(_p(claims), len(claims), C.byref(h))
    if rc != 0:
        raise EngineError(f"compact_storage_claims: {lib.ipcfp_strerror(rc).decode()} ({rc})")
    return StorageColumns(h)


def expand_storage_claims(cols: StorageColumns) -> np.ndarray:
    """Host-only: the column form → SCLAIM_DTYPE[n] (ipcfp_expand_storage_claims)."""
    lib = load_library()
    out = np.zeros(cols.n, dtype=SCLAIM_DTYPE)
    rc = lib.ipcfp_expand_storage_claims(cols.h, _p(out))
    if rc != 0:
        raise EngineError(f"expand_storage_claims: {lib.ipcfp_strerror(rc).decode()} ({rc})")
    return out


class EventProofStruct(C.Structure):
    """ipcfp_event_proof_t (include/ipcfp.h): the view UnpackedEvents / GeneratedEvents.proofs() hand out."""

    _fields_ = [("parent_epoch", C.c_int64), ("child_epoch", C.c_int64), ("parent_tipset_cids", C.POINTER(C.c_char_p)),
                ("n_parent_tipset_cids", C.c_uint32), ("child_block_cid", C.c_char_p), ("message_cid", C.c_char_p),
                ("exec_index", C.c_uint64), ("event_index", C.c_uint64), ("emitter", C.c_uint64),
                ("topics", C.POINTER(C.c_char_p)), ("n_topics", C.c_uint32), ("data", C.c_char_p)]


def _proof_rows(ptr: int, n: int):
    """ipcfp_event_proof_t[n] at an address → a list of dicts holding Python copies of every field (no pointer survives)."""
    arr = (EventProofStruct * n).from_address(ptr) if n else []
    rows = []
    for p in arr:
        rows.append({"parent_epoch": p.parent_epoch, "child_epoch": p.child_epoch,
                     "parent_tipset_cids": [p.parent_tipset_cids[k].decode() for k in range(p.n_parent_tipset_cids)],
                     "child_block_cid": p.child_block_cid.decode(), "message_cid": p.message_cid.decode(),
                     "exec_index": p.exec_index, "event_index": p.event_index, "emitter": p.emitter,
                     "topics": [p.topics[k].decode() for k in range(p.n_topics)], "data": p.data.decode()})
    return rows


class UnpackedEvents:
    """EventProof structs with the reference's strings (ipcfp_unpacked_events_t): owns the handle; `ptr` / `n` are the
    ipcfp_event_proof_t array (valid until close()) for the entry points that take claim structs."""

    def __init__(self, handle):
        self.lib = load_library()
        self.h = handle
        n = C.c_uint64()
        self.ptr = self.lib.ipcfp_unpacked_events_proofs(handle, C.byref(n)) or 0
        self.n = int(n.value)

    def rows(self):
        return _proof_rows(self.ptr, self.n)

    def close(self):
        if self.h:
            self.lib.ipcfp_unpacked_events_destroy(self.h)
            self.h = None
            self.ptr = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def unpack_event_claims(tipsets: np.ndarray, claims: np.ndarray, blob: np.ndarray, blob_len=None) -> UnpackedEvents:
    """Host-only inverse of pack_event_proofs (ipcfp_unpack_event_claims; no GPU): packed claims → EventProof structs.
    A refusal raises EngineError with `.rc` (the IPCFP_E_* code) and `.bad_index` (the lowest offending claim)."""
    lib = load_library()
    ts = np.ascontiguousarray(tipsets, dtype=TIPSET_DTYPE)
    cl = np.ascontiguousarray(claims, dtype=CLAIM_DTYPE)
    bl = np.ascontiguousarray(blob, dtype=np.uint8)
    h, bad = C.c_void_p(), C.c_uint64()
    rc = lib.ipcfp_unpack_event_claims(_p(ts) if len(ts) else None, len(ts), _p(cl) if len(cl) else None, len(cl),
                                       _p(bl) if len(bl) else None, len(bl) if blob_len is None else int(blob_len), C.byref(h),
                                       C.byref(bad))
    if rc != 0:
        e = EngineError(f"unpack_event_claims: claim {bad.value}: {lib.ipcfp_strerror(rc).decode()} ({rc})")
        e.rc, e.bad_index = rc, int(bad.value)
        raise e
    return UnpackedEvents(h)


class GeneratedEvents:
    """The proofs of one generate_event_proof call as packed claims resident in HBM (ipcfp_generated_events_t): owns the
    handle — close it before the engine.  `claims_ptr` / `blob_ptr` / `blob_len` / `tipsets` are what
    Witness.verify_event_claims_device takes."""

    def __init__(self, eng: "Engine", handle):
        self.eng = eng
        self.lib = eng.lib
        self.h = handle
        lib = self.lib
        self.n = int(lib.ipcfp_generated_events_count(handle))
        bl = C.c_uint64()
        self.claims_ptr = lib.ipcfp_generated_events_claims_device(handle) or 0
        self.blob_ptr = lib.ipcfp_generated_events_blob_device(handle, C.byref(bl)) or 0
        self.blob_len = int(bl.value)
        # one record per INPUT tipset (the single call: one); more_parents points into the handle
        nt = C.c_uint32()
        pt = lib.ipcfp_generated_events_tipsets(handle, C.byref(nt))
        self.tipset_count = int(lib.ipcfp_generated_events_tipset_count(handle))
        buf = (C.c_uint8 * (TIPSET_DTYPE.itemsize * nt.value)).from_address(pt)
        self.tipsets = np.frombuffer(buf, dtype=TIPSET_DTYPE)
        ps = lib.ipcfp_generated_events_tipset_status(handle, C.byref(nt))
        self.tipset_status = np.frombuffer((C.c_uint8 * nt.value).from_address(ps), dtype=np.uint8).copy()
        po = lib.ipcfp_generated_events_tipset_claim_off(handle, C.byref(nt))
        self.tipset_claim_off = np.frombuffer((C.c_uint8 * (8 * (nt.value + 1))).from_address(po), dtype=np.uint64).copy()
        nb = C.c_uint64()
        pb = lib.ipcfp_generated_events_block_ids(handle, C.byref(nb))
        self.block_ids = (np.frombuffer((C.c_uint8 * (4 * nb.value)).from_address(pb), dtype=np.uint32).copy() if nb.value
                          else np.zeros(0, np.uint32))

    def copy(self):
        """→ (claims CLAIM_DTYPE[n], blob u8[blob_len]) on the host."""
        claims = np.zeros(self.n, dtype=CLAIM_DTYPE)
        blob = np.zeros(self.blob_len, dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_generated_events_copy(self.h, _p(claims) if self.n else None,
                                                             _p(blob) if self.blob_len else None, self.blob_len),
                        "generated_events_copy")
        return claims, blob

    def matches(self):
        """→ (match records MATCH_DTYPE[n], message CID slots u8[n, 40]) on the host."""
        n = C.c_uint64()
        pm = self.lib.ipcfp_generated_events_matches(self.h, C.byref(n))
        pc = self.lib.ipcfp_generated_events_message_cids(self.h, C.byref(n))
        if pm is None and pc is None and self.n:
            self.eng._check(-3, "generated_events_matches")
        if not self.n:
            return np.zeros(0, dtype=MATCH_DTYPE), np.zeros((0, CID_SLOT), dtype=np.uint8)
        m = np.frombuffer((C.c_uint8 * (MATCH_DTYPE.itemsize * self.n)).from_address(pm), dtype=MATCH_DTYPE).copy()
        c = np.frombuffer((C.c_uint8 * (CID_SLOT * self.n)).from_address(pc), dtype=np.uint8).reshape(-1, CID_SLOT).copy()
        return m, c

    def proofs(self):
        """→ (address of ipcfp_event_proof_t[n], n): the reference's strings, owned by the handle (valid until close()).
        EngineError with `.rc` / `.bad_index` when a proof has no string form (a folded CID: IPCFP_E_UNSUPPORTED)."""
        p, n, bad = C.c_void_p(), C.c_uint64(), C.c_uint64()
        rc = self.lib.ipcfp_generated_events_proofs(self.h, C.byref(p), C.byref(n), C.byref(bad))
        if rc != 0:
            msg = self.lib.ipcfp_last_error(self.eng.h)
            e = EngineError(f"generated_events_proofs: {msg.decode() if msg else ''} ({rc})")
            e.rc, e.bad_index = rc, int(bad.value)
            raise e
        return (p.value or 0), int(n.value)

    def proof_rows(self):
        return _proof_rows(*self.proofs())

    def close(self):
        if getattr(self, "h", None):
            self.tipsets = None
            if self.eng.h:  # a context that is already gone took its device memory with it
                self.lib.ipcfp_generated_events_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StorageProofStruct(C.Structure):
    """ipcfp_storage_proof_t (include/ipcfp.h): the view UnpackedStorage / GeneratedStorageClaims.proofs() hand out."""

    _fields_ = [("child_epoch", C.c_int64), ("child_block_cid", C.c_char_p), ("parent_state_root", C.c_char_p),
                ("actor_id", C.c_uint64), ("actor_state_cid", C.c_char_p), ("storage_root", C.c_char_p), ("slot", C.c_char_p),
                ("value", C.c_char_p)]


def _storage_proof_rows(ptr: int, n: int):
    """ipcfp_storage_proof_t[n] at an address → a list of dicts holding Python copies of every field."""
    arr = (StorageProofStruct * n).from_address(ptr) if n else []
    return [{"child_epoch": p.child_epoch, "child_block_cid": p.child_block_cid.decode(),
             "parent_state_root": p.parent_state_root.decode(), "actor_id": p.actor_id,
             "actor_state_cid": p.actor_state_cid.decode(), "storage_root": p.storage_root.decode(), "slot": p.slot.decode(),
             "value": p.value.decode()} for p in arr]


class UnpackedStorage:
    """StorageProof structs with the reference's strings (ipcfp_unpacked_storage_t): owns the handle; `ptr` / `n` are the
    ipcfp_storage_proof_t array (valid until close()) for the entry points that take claim structs."""

    def __init__(self, handle):
        self.lib = load_library()
        self.h = handle
        n = C.c_uint64()
        self.ptr = self.lib.ipcfp_unpacked_storage_proofs(handle, C.byref(n)) or 0
        self.n = int(n.value)

    def rows(self):
        return _storage_proof_rows(self.ptr, self.n)

    def close(self):
        if self.h:
            self.lib.ipcfp_unpacked_storage_destroy(self.h)
            self.h = None
            self.ptr = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def unpack_storage_claims(claims: np.ndarray) -> UnpackedStorage:
    """Host-only inverse of pack_storage_proofs (ipcfp_unpack_storage_claims; no GPU): SCLAIM_DTYPE[n] → StorageProof structs.
    A refusal raises EngineError with `.rc` (the IPCFP_E_* code) and `.bad_index` (the lowest offending claim)."""
    lib = load_library()
    cl = np.ascontiguousarray(claims, dtype=SCLAIM_DTYPE)
    h, bad = C.c_void_p(), C.c_uint64()
    rc = lib.ipcfp_unpack_storage_claims(_p(cl) if len(cl) else None, len(cl), C.byref(h), C.byref(bad))
    if rc != 0:
        e = EngineError(f"unpack_storage_claims: claim {bad.value}: {lib.ipcfp_strerror(rc).decode()} ({rc})")
        e.rc, e.bad_index = rc, int(bad.value)
        raise e
    return UnpackedStorage(h)


class GeneratedStorageClaims:
    """The proofs of one batch of generate_storage_proof specs as column claims resident in HBM
    (ipcfp_generated_storage_claims_t): owns the handle — close it before the engine.  `runs_ptr` / `n_runs` / `slot_ptr` /
    `value_ptr` / `cflags_ptr` / `n` are what Witness.verify_storage_columns_device and expand_storage_claims_device take."""

    def __init__(self, eng: "Engine", handle):
        self.eng = eng
        self.lib = eng.lib
        self.h = handle
        lib = self.lib
        self.n = int(lib.ipcfp_generated_storage_claims_count(handle))
        self.n_runs = int(lib.ipcfp_generated_storage_claims_run_count(handle))
        self.runs_ptr = lib.ipcfp_generated_storage_claims_runs_device(handle) or 0
        self.slot_ptr = lib.ipcfp_generated_storage_claims_slots_device(handle) or 0
        self.value_ptr = lib.ipcfp_generated_storage_claims_values_device(handle) or 0
        self.cflags_ptr = lib.ipcfp_generated_storage_claims_cflags_device(handle) or 0
        self.status_ptr = lib.ipcfp_generated_storage_claims_status_device(handle) or 0
        nb = C.c_uint64()
        pb = lib.ipcfp_generated_storage_claims_block_ids(handle, C.byref(nb))
        self.block_ids = (np.frombuffer((C.c_uint8 * (4 * nb.value)).from_address(pb), dtype=np.uint32).copy() if nb.value
                          else np.zeros(0, np.uint32))

    def status(self) -> np.ndarray:
        """→ one status byte per spec (a host copy)."""
        n = C.c_uint64()
        ps = self.lib.ipcfp_generated_storage_claims_status(self.h, C.byref(n))
        if not self.n:
            return np.zeros(0, np.uint8)
        if not ps:
            self.eng._check(-3, "generated_storage_claims_status")
        return np.frombuffer((C.c_uint8 * self.n).from_address(ps), dtype=np.uint8).copy()

    @property
    def first_error(self):
        """Index of the first spec whose status is not 1, or None."""
        v = int(self.lib.ipcfp_generated_storage_claims_first_error(self.h))
        return None if v == 2**64 - 1 else v

    @property
    def n_tipsets(self) -> int:
        """Children of the chain the handle answers (generate_storage_claims_tipsets*); 1 for a single-child handle."""
        return int(self.lib.ipcfp_generated_storage_claims_tipset_count(self.h))

    def tipset_first_error(self, t: int):
        """Index WITHIN tipset t of its first spec whose status is not 1, or None."""
        if not 0 <= t < self.n_tipsets:
            raise IndexError(t)
        v = int(self.lib.ipcfp_generated_storage_claims_tipset_first_error(self.h, t))
        return None if v == 2**64 - 1 else v

    def tipset_block_ids(self, t: int) -> np.ndarray:
        """The blocks tipset t alone recorded, in `Cid: Ord` order: what a single call for that child returns."""
        if not 0 <= t < self.n_tipsets:
            raise IndexError(t)
        nb = C.c_uint64()
        pb = self.lib.ipcfp_generated_storage_claims_tipset_block_ids(self.h, t, C.byref(nb))
        if not nb.value:
            return np.zeros(0, np.uint32)
        return np.frombuffer((C.c_uint8 * (4 * nb.value)).from_address(pb), dtype=np.uint32).copy()

    def copy(self):
        """→ (runs record[n_runs], slot u8[n, 32], value u8[n, 32], cflags u8[n]) on the host."""
        runs = np.zeros(self.n_runs, dtype=_SRUN_DTYPE)
        slot = np.zeros((self.n, 32), dtype=np.uint8)
        value = np.zeros((self.n, 32), dtype=np.uint8)
        cflags = np.zeros(self.n, dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_generated_storage_claims_copy(self.h, _p(runs) if self.n_runs else None,
                                                                     _p(slot) if self.n else None, _p(value) if self.n else None,
                                                                     _p(cflags) if self.n else None), "generated_storage_claims_copy")
        return runs, slot, value, cflags

    def proofs(self):
        """→ (address of ipcfp_storage_proof_t[n], n): the reference's strings, owned by the handle (valid until close()).
        EngineError with `.rc` / `.bad_index`: IPCFP_E_INVALID at the first failing spec, IPCFP_E_UNSUPPORTED at the first
        proof with a folded CID."""
        p, n, bad = C.c_void_p(), C.c_uint64(), C.c_uint64()
        rc = self.lib.ipcfp_generated_storage_claims_proofs(self.h, C.byref(p), C.byref(n), C.byref(bad))
        if rc != 0:
            msg = self.lib.ipcfp_last_error(self.eng.h)
            e = EngineError(f"generated_storage_claims_proofs: {msg.decode() if msg else ''} ({rc})")
            e.rc, e.bad_index = rc, int(bad.value)
            raise e
        return (p.value or 0), int(n.value)

    def proof_rows(self):
        return _storage_proof_rows(*self.proofs())

    def close(self):
        if getattr(self, "h", None):
            if self.eng.h:  # a context that is already gone took its device memory with it
                self.lib.ipcfp_generated_storage_claims_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bundle_check_json(text: bytes, flags: int = 0):
    """Host half of the bundle parse (no GPU): → (ok, n_storage, n_events, n_blocks, error text)."""
    lib = load_library()
    text = bytes(text)
    ns, ne, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    err = C.create_string_buffer(256)
    rc = lib.ipcfp_bundle_check_json(text, len(text), flags, C.byref(ns), C.byref(ne), C.byref(nb), err, 256)
    return rc == 0, int(ns.value), int(ne.value), int(nb.value), err.value.decode(errors="replace")


def _claims_ptr(arr):
    """A ctypes array of claim structs, an address, or None → c_void_p"""
    if arr is None or isinstance(arr, (int, C.c_void_p)):
        return arr
    return C.cast(arr, C.c_void_p)


def bundle_claims_json(storage_arr, n_storage: int, event_arr, n_events: int) -> bytes:
    """The head of a bundle's JSON text, `{"storage_proofs":[…],"event_proofs":[…],"blocks":[`, as serde_json writes it
    (ipcfp_bundle_write_claims_json: host only, no engine).  The arrays are ctypes arrays of the ipcfp.h claim structs."""
    lib = load_library()
    sp, ep = _claims_ptr(storage_arr), _claims_ptr(event_arr)
    n = C.c_uint64()
    rc = lib.ipcfp_bundle_write_claims_json(sp, n_storage, ep, n_events, None, 0, C.byref(n))
    if rc != 0:
        raise EngineError(f"bundle_write_claims_json: {lib.ipcfp_strerror(rc).decode()} ({rc})")
    buf = C.create_string_buffer(max(int(n.value), 1))
    rc = lib.ipcfp_bundle_write_claims_json(sp, n_storage, ep, n_events, C.cast(buf, C.c_void_p), n.value, C.byref(n))
    if rc != 0:
        raise EngineError(f"bundle_write_claims_json: {lib.ipcfp_strerror(rc).decode()} ({rc})")
    return buf.raw[: int(n.value)]


class Bundle:
    """A parsed `UnifiedProofBundle` JSON (``ipcfp_bundle_t``): witness in HBM + the claim structs."""

    CID_STRINGS = 1

    def __init__(self, eng: "Engine", text: bytes, flags: int = 0):
        self.eng = eng
        self.lib = eng.lib
        h = C.c_void_p()
        text = bytes(text)
        eng._check(self.lib.ipcfp_bundle_parse_json(eng.h, text, len(text), flags, C.byref(h)), "bundle_parse_json")
        self.h = h
        self.n_blocks = int(self.lib.ipcfp_bundle_block_count(h))
        self.n_events = int(self.lib.ipcfp_bundle_event_count(h))
        self.n_storage = int(self.lib.ipcfp_bundle_storage_count(h))
        w = Witness.__new__(Witness)  # a view: the bundle owns the witness
        w.eng, w.lib, w.h, w.n, w._borrowed = eng, eng.lib, C.c_void_p(self.lib.ipcfp_bundle_witness(h)), self.n_blocks, True
        self.witness = w

    def verify(self, trust=None, filt=None):
        """verify_proof_bundle → (storage_status u8[], event_status u8[])."""
        ss = np.zeros(max(self.n_storage, 1), dtype=np.uint8)
        es = np.zeros(max(self.n_events, 1), dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_verify_proof_bundle(
            self.eng.h, self.h, C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            C.cast(C.pointer(filt), C.c_void_p) if filt is not None else None, _p(ss), _p(es)), "verify_proof_bundle")
        return ss[: self.n_storage], es[: self.n_events]

    def to_json(self) -> bytes:
        """The bundle back as its JSON wire form: its own claim structs and every block of its witness in id order."""
        return self.witness.write_bundle_json(self.lib.ipcfp_bundle_storage_proofs(self.h), self.n_storage,
                                              self.lib.ipcfp_bundle_event_proofs(self.h), self.n_events)

    def close(self):
        if getattr(self, "h", None):
            self.witness.h = None
            if self.eng.h:  # a context that is already gone took its device memory with it
                self.lib.ipcfp_bundle_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Witness:
    """HBM-resident witness store (``ipcfp_witness_t``)."""

    def __init__(self, eng: Engine, data, off, lens, cids40, device=None, packed=None):
        self.eng = eng
        self.lib = eng.lib
        h = C.c_void_p()
        if packed is not None:
            pk = packed
            n = len(pk.lens)
            rc = self.lib.ipcfp_witness_create_packed(eng.h, _p(pk.data), pk.data.size, _p(pk.lens), _p(pk.digests), n,
                                                      _p(pk.prefix), len(pk.prefix), _p(pk.esc_index), _p(pk.esc_cids),
                                                      len(pk.esc_index), C.byref(h))
        elif device is None:
            data = np.ascontiguousarray(data, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            lens = np.ascontiguousarray(lens, dtype=np.uint32)
            cids40 = np.ascontiguousarray(cids40, dtype=np.uint8).reshape(-1, CID_SLOT)
            n = len(off)
            if len(lens) != n or len(cids40) != n:
                raise EngineError("off/len/cids length mismatch")
            rc = self.lib.ipcfp_witness_create(eng.h, _p(data), data.size, _p(off), _p(lens), _p(cids40), n, C.byref(h))
        else:
            bp, nbytes, op, lp, cp, n = device
            rc = self.lib.ipcfp_witness_create_device(eng.h, bp, nbytes, op, lp, cp, n, C.byref(h))
        eng._check(rc, "witness_create")
        self.h = h
        self.n = int(n)

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False) and self.eng.h:
                self.lib.ipcfp_witness_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def block_count(self) -> int:
        return int(self.lib.ipcfp_witness_block_count(self.h))

    def write_bundle_json(self, storage_ptr, n_storage: int, event_ptr, n_events: int, block_ids=None) -> bytes:
        """`serde_json::to_string(&UnifiedProofBundle)` of the given claims (ctypes arrays of the ipcfp.h structs, or
        addresses) and the listed blocks of this witness (None: every block in id order); base64 on the device."""
        sp, ep = _claims_ptr(storage_ptr), _claims_ptr(event_ptr)
        if block_ids is None:
            ids, nb = None, self.n
        else:
            ids = np.ascontiguousarray(block_ids, dtype=np.uint32)
            nb = len(ids)
        n = C.c_uint64()
        args = (self.eng.h, self.h, sp, n_storage, ep, n_events, _p(ids), nb)
        self.eng._check(self.lib.ipcfp_bundle_write_json(*args, None, 0, C.byref(n)), "bundle_write_json")
        out = np.empty(int(n.value), dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_bundle_write_json(*args, _p(out), out.size, C.byref(n)), "bundle_write_json")
        return out.tobytes()

    def verify_cids(self):
        """K1.  Returns (status u8[n], n_bad)."""
        st = np.zeros(self.n, dtype=np.uint8)
        bad = C.c_uint64()
        self.eng._check(self.lib.ipcfp_witness_verify_cids(self.eng.h, self.h, _p(st), C.byref(bad)), "verify_cids")
        return st, int(bad.value)

    def cid_results(self, want_status=True):
        """(status u8[n] | None, n_bad) of the last verify_cids_async — waits for it, launches nothing."""
        st = np.zeros(self.n, dtype=np.uint8) if want_status else None
        bad = C.c_uint64()
        self.eng._check(self.lib.ipcfp_witness_cid_results(self.eng.h, self.h, _p(st), C.byref(bad)), "cid_results")
        return st, int(bad.value)

    def verify_cids_async(self):
        self.eng._check(self.lib.ipcfp_witness_verify_cids_async(self.eng.h, self.h), "verify_cids_async")

    # -- path-walk primitives ---------------------------------------------------------
    def amt_get(self, root_cid: bytes, version: int, kind: str, indices):
        """K5.  Returns (status u8[n], loc structured[n] with fields block/off/len)."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        n = len(idx)
        st = np.zeros(n, dtype=np.uint8)
        loc = np.zeros(n, dtype=LOC_DTYPE)
        root = cid_slots([root_cid])[0].copy()
        self.eng._check(self.lib.ipcfp_amt_get(self.eng.h, self.h, _p(root), version, VALUE_KINDS[kind], _p(idx), n,
                                               _p(st), _p(loc)), "amt_get")
        return st, loc

    def hamt_get(self, root_cid: bytes, bit_width: int, kind: str, keys):
        """K7.  keys: list[bytes]."""
        n = len(keys)
        kl = np.array([len(k) for k in keys], dtype=np.uint32)
        ko = np.zeros(n, dtype=np.uint32)
        if n:
            ko[1:] = np.cumsum(kl[:-1])
        kb = np.frombuffer(b"".join(keys), dtype=np.uint8).copy() if n and kl.sum() else np.zeros(1, np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        loc = np.zeros(n, dtype=LOC_DTYPE)
        root = cid_slots([root_cid])[0].copy()
        self.eng._check(self.lib.ipcfp_hamt_get(self.eng.h, self.h, _p(root), bit_width, VALUE_KINDS[kind], _p(kb),
                                                _p(ko), _p(kl), n, _p(st), _p(loc)), "hamt_get")
        return st, loc

    def hamt_get_device(self, root_cid: bytes, bit_width: int, kind: str, keys_ptr: int, key_off_ptr: int, key_len_ptr: int,
                        n: int, status_ptr: int, loc_ptr: int = 0):
        """K7 with every buffer resident in HBM; asynchronous (eng.sync() completes it)."""
        root = cid_slots([root_cid])[0].copy()
        self.eng._check(self.lib.ipcfp_hamt_get_device(self.eng.h, self.h, _p(root), bit_width, VALUE_KINDS[kind], keys_ptr,
                                                       key_off_ptr, key_len_ptr, int(n), status_ptr, loc_ptr or None),
                        "hamt_get_device")

    def exec_order(self, parent_cids, cap=None):
        """reconstruct_execution_order → (status, cids u8[count, 40])."""
        pc = np.zeros((max(len(parent_cids), 1), CID_SLOT), dtype=np.uint8)
        pc[: len(parent_cids)] = cid_slots(parent_cids)
        st = np.zeros(1, dtype=np.uint8)
        cnt = C.c_uint64()
        # first call: count only
        self.eng._check(self.lib.ipcfp_exec_order(self.eng.h, self.h, _p(pc), len(parent_cids), _p(st), None, 0,
                                                  C.byref(cnt)), "exec_order")
        n = int(cnt.value) if cap is None else min(int(cnt.value), cap)
        out = np.zeros((n, CID_SLOT), dtype=np.uint8)
        if n:
            self.eng._check(self.lib.ipcfp_exec_order(self.eng.h, self.h, _p(pc), len(parent_cids), _p(st), _p(out), n,
                                                      C.byref(cnt)), "exec_order")
        return int(st[0]), out

    def scan_events(self, receipts_root: bytes, topic0: bytes, topic1: bytes, actor=None, want_touched=True,
                    counts_only=False, caps=None):
        """K6/K8.  Returns (status, has_match u8[n_receipts], matches structured[n], touched block ids);
        with counts_only: (status, n_receipts, n_matches, None) and nothing is copied back.
        caps = (cap_receipts, cap_matches): ONE call into buffers of that size instead of a sizing call followed by
        the real one (a host that knows its tipset's receipt count); falls back to the two-call form on overflow."""
        # (the marshalled arguments of the last call are kept: a scan repeated with the same filter — a service polling
        # one subnet's events, the benchmark's step — pays for the numpy / ctypes conversions once)
        key = (bytes(receipts_root), bytes(topic0), bytes(topic1))
        cached = getattr(self, "_scan_args", None)
        if cached is None or cached[0] != key:
            root = np.frombuffer(key[0].ljust(CID_SLOT, b"\0"), dtype=np.uint8).copy()
            filt = np.frombuffer(key[1] + key[2], dtype=np.uint8).copy()
            st = np.zeros(1, dtype=np.uint8)
            nr, nm = C.c_uint64(), C.c_uint64()
            cached = (key, root, filt, st, nr, nm, _p(root), _p(filt), _p(st), C.byref(nr), C.byref(nm))
            self._scan_args = cached
        _, root, filt, st, nr, nm, p_root, p_filt, p_st, r_nr, r_nm = cached
        a = (0, 0) if actor is None else (1, int(actor))
        if caps is not None and not counts_only and not want_touched:
            has = np.zeros(int(caps[0]), dtype=np.uint8)
            m = np.zeros(int(caps[1]), dtype=MATCH_DTYPE)
            self.eng._check(self.lib.ipcfp_scan_events(self.eng.h, self.h, p_root, p_filt, a[0], a[1], p_st, _p(has), len(has),
                                                       r_nr, _p(m), len(m), r_nm, None), "scan_events")
            if st[0] != 1 or (nr.value <= len(has) and nm.value <= len(m)):
                return int(st[0]), has[: int(nr.value)], m[: int(nm.value)], None
        # sizing call, then the real one
        self.eng._check(self.lib.ipcfp_scan_events(self.eng.h, self.h, p_root, p_filt, a[0], a[1], p_st, None, 0,
                                                   r_nr, None, 0, r_nm, None), "scan_events")
        if counts_only:
            return int(st[0]), int(nr.value), int(nm.value), None
        words = (self.n + 31) // 32
        touched = np.zeros(max(words, 1), dtype=np.uint32) if want_touched else None
        has = np.zeros(int(nr.value), dtype=np.uint8)
        m = np.zeros(int(nm.value), dtype=MATCH_DTYPE)
        if st[0] == 1:
            self.eng._check(self.lib.ipcfp_scan_events(self.eng.h, self.h, _p(root), _p(filt), a[0], a[1], _p(st),
                                                       _p(has), len(has), C.byref(nr), _p(m), len(m), C.byref(nm),
                                                       _p(touched)), "scan_events")
        ids = None
        if want_touched:
            bits = np.unpackbits(touched.view(np.uint8), bitorder="little")[: self.n]
            ids = np.nonzero(bits)[0]
        return int(st[0]), has, m, ids

    def last_scan_phase(self) -> int:
        """Where the Err of the last scan on this witness arose: 0 (it returned TRUE), SCAN_PHASE_RECEIPTS (the enumeration of
        the tipset's receipts, which precedes every events AMT) or SCAN_PHASE_EVENTS — what a merge of receipt-range shards
        needs to name the unsharded call's Err (merge_scan_status)."""
        return int(self.eng.lib.ipcfp_witness_last_scan_phase(self.h))

    def scan_events_device(self, receipts_root: bytes, topic0: bytes, topic1: bytes, actor, has_ptr: int, cap_receipts: int,
                           matches_ptr: int = 0, cap_matches: int = 0, summary_ptr: int = 0):
        """K6 with device outputs (has-match map / match records stay in HBM).  → (status, n_receipts, n_matches)"""
        root = cid_slots([receipts_root])[0].copy()
        filt = np.frombuffer(bytes(topic0) + bytes(topic1), dtype=np.uint8).copy()
        st = np.zeros(1, dtype=np.uint8)
        nr, nm = C.c_uint64(), C.c_uint64()
        a = (0, 0) if actor is None else (1, int(actor))
        self.eng._check(self.lib.ipcfp_scan_events_device(self.eng.h, self.h, _p(root), _p(filt), a[0], a[1], _p(st),
                                                          has_ptr or None, int(cap_receipts), C.byref(nr),
                                                          matches_ptr or None, int(cap_matches), C.byref(nm),
                                                          summary_ptr or None), "scan_events_device")
        return int(st[0]), int(nr.value), int(nm.value)

    @staticmethod
    def _scan_specs(specs):
        """[(topic0, topic1, actor or None)] → (filters u8[n, 64], has_actor u8[n], actors u64[n])"""
        filt = np.zeros((len(specs), 64), dtype=np.uint8)
        has = np.zeros(len(specs), dtype=np.uint8)
        actors = np.zeros(len(specs), dtype=np.uint64)
        for j, (t0, t1, actor) in enumerate(specs):
            key = bytes(t0) + bytes(t1)
            if len(key) != 64:
                raise ValueError(f"spec {j}: topic0 and topic1 are 32 bytes each")
            filt[j] = np.frombuffer(key, dtype=np.uint8)
            if actor is not None:
                has[j], actors[j] = 1, int(actor)
        return filt, has, actors

    def scan_events_multi(self, receipts_root: bytes, specs, want_touched=True, cap_matches=None):
        """The scan for a SET of specs [(topic0, topic1, actor or None)] in one pass (ipcfp_scan_events_multi).
        → (status, has_match u8[n_receipts] — some spec matches —, matches structured[n], match_spec u32[n], spec_counts
        u64[n_specs], touched block ids, per_spec) where per_spec[j] = matches[match_spec == j], spec j's own match list.
        cap_matches: at most that many records come back (the counts stay the full ones); None: all of them."""
        root = cid_slots([receipts_root])[0].copy()
        filt, has_a, actors = self._scan_specs(specs)
        n = len(specs)
        st = np.zeros(1, dtype=np.uint8)
        nr, nm = C.c_uint64(), C.c_uint64()
        counts = np.zeros(max(n, 1), dtype=np.uint64)

        def call(has, m, ms, touched):
            self.eng._check(self.lib.ipcfp_scan_events_multi(self.eng.h, self.h, _p(root), _p(filt), _p(has_a), _p(actors), n, _p(st),
                                                             _p(has), 0 if has is None else len(has), C.byref(nr),
                                                             _p(m), _p(ms), 0 if m is None else len(m), C.byref(nm),
                                                             _p(counts), _p(touched)), "scan_events_multi")

        call(None, None, None, None)  # the sizing call
        if st[0] != 1:
            return int(st[0]), None, None, None, None, None, None
        total = int(nm.value)
        take = total if cap_matches is None else min(total, int(cap_matches))
        has = np.zeros(int(nr.value), dtype=np.uint8)
        m = np.zeros(take, dtype=MATCH_DTYPE) if take else None
        ms = np.zeros(take, dtype=np.uint32) if take else None
        touched = np.zeros(max((self.n + 31) // 32, 1), dtype=np.uint32) if want_touched else None
        call(has, m, ms, touched)
        m = np.zeros(0, dtype=MATCH_DTYPE) if m is None else m
        ms = np.zeros(0, dtype=np.uint32) if ms is None else ms
        ids = None
        if want_touched:
            ids = np.nonzero(np.unpackbits(touched.view(np.uint8), bitorder="little")[: self.n])[0]
        per_spec = [m[ms == j] for j in range(n)]
        return int(st[0]), has, m, ms, counts[:n].copy(), ids, per_spec

    def scan_events_multi_device(self, receipts_root: bytes, specs, has_ptr: int = 0, cap_receipts: int = 0, matches_ptr: int = 0,
                                 match_spec_ptr: int = 0, cap_matches: int = 0, spec_counts_ptr: int = 0, summary_ptr: int = 0):
        """ipcfp_scan_events_multi_device: the map, the records, match_spec and the per-spec counts stay in HBM (pointers of
        the caller, 0: not wanted).  → (status, n_receipts, n_matches)"""
        root = cid_slots([receipts_root])[0].copy()
        filt, has_a, actors = self._scan_specs(specs)
        st = np.zeros(1, dtype=np.uint8)
        nr, nm = C.c_uint64(), C.c_uint64()
        self.eng._check(self.lib.ipcfp_scan_events_multi_device(self.eng.h, self.h, _p(root), _p(filt), _p(has_a), _p(actors), len(specs),
                                                                _p(st), has_ptr or None, int(cap_receipts), C.byref(nr),
                                                                matches_ptr or None, match_spec_ptr or None, int(cap_matches),
                                                                C.byref(nm), spec_counts_ptr or None, summary_ptr or None),
                        "scan_events_multi_device")
        return int(st[0]), int(nr.value), int(nm.value)

    def scan_events_tipsets(self, receipts_roots, specs, want_touched=True, cap_matches=None, cap_receipts=None):
        """The scan of a CHAIN of tipsets for a set of specs in one pass (ipcfp_scan_events_tipsets): what
        [scan_events_multi(root, specs) for root in receipts_roots] answers, laid end to end.  → a dict:
          status u8[T], phase u8[T]       per tipset (phase 0 with status 1)
          receipt_off, match_off u64[T+1] never truncated; n_receipts, n_matches: their last entries
          has_match u8, matches structured, match_spec u32   the concatenated arrays, cut to cap_receipts / cap_matches
          spec_counts u64[n_specs], touched (block ids, None without want_touched)
          maps, records, record_specs     per tipset, split by the offsets (what the capacities cut away is missing);
                                          a failing tipset's are empty
        The ABI call is made TWICE — a sizing call, then the call that takes the outputs — and each is a whole pass (an
        enumeration and both passes over the chain); when the sizing call shows nothing to fetch (no map byte and no record
        inside the capacities, no recorder asked for) the second call is not made.  A caller that knows its capacities
        uses scan_events_tipsets_device, one pass."""
        roots = cid_slots(list(receipts_roots)).copy() if len(receipts_roots) else np.zeros((0, CID_SLOT), dtype=np.uint8)
        filt, has_a, actors = self._scan_specs(specs)
        T, n = len(receipts_roots), len(specs)
        st = np.zeros(max(T, 1), dtype=np.uint8)
        ph = np.zeros(max(T, 1), dtype=np.uint8)
        roff = np.zeros(T + 1, dtype=np.uint64)
        moff = np.zeros(T + 1, dtype=np.uint64)
        nr, nm = C.c_uint64(), C.c_uint64()
        counts = np.zeros(max(n, 1), dtype=np.uint64)

        def call(has, m, ms, touched):
            self.eng._check(self.lib.ipcfp_scan_events_tipsets(self.eng.h, self.h, _p(roots), T, _p(filt), _p(has_a), _p(actors), n,
                                                               _p(st), _p(ph), _p(roff), _p(moff),
                                                               _p(has), 0 if has is None else len(has), C.byref(nr),
                                                               _p(m), _p(ms), 0 if m is None else len(m), C.byref(nm),
                                                               _p(counts), _p(touched)), "scan_events_tipsets")

        call(None, None, None, None)  # the sizing call
        total_r, total_m = int(nr.value), int(nm.value)
        take_r = total_r if cap_receipts is None else min(total_r, int(cap_receipts))
        take_m = total_m if cap_matches is None else min(total_m, int(cap_matches))
        has = np.zeros(take_r, dtype=np.uint8) if take_r else None
        m = np.zeros(take_m, dtype=MATCH_DTYPE) if take_m else None
        ms = np.zeros(take_m, dtype=np.uint32) if take_m else None
        touched = np.zeros(max((self.n + 31) // 32, 1), dtype=np.uint32) if want_touched else None
        if take_r or take_m or want_touched:  # (else the sizing call has answered: statuses, offsets, totals, spec_counts)
            call(has, m, ms, touched)
        has = np.zeros(0, dtype=np.uint8) if has is None else has
        m = np.zeros(0, dtype=MATCH_DTYPE) if m is None else m
        ms = np.zeros(0, dtype=np.uint32) if ms is None else ms
        ids = None
        if want_touched:
            ids = np.nonzero(np.unpackbits(touched.view(np.uint8), bitorder="little")[: self.n])[0]
        r, o = [int(v) for v in roff], [int(v) for v in moff]
        return {
            "status": st[:T].copy(), "phase": ph[:T].copy(), "receipt_off": roff, "match_off": moff,
            "n_receipts": int(nr.value), "n_matches": int(nm.value), "has_match": has, "matches": m, "match_spec": ms,
            "spec_counts": counts[:n].copy(), "touched": ids,
            "maps": [has[min(r[t], take_r):min(r[t + 1], take_r)] for t in range(T)],
            "records": [m[min(o[t], take_m):min(o[t + 1], take_m)] for t in range(T)],
            "record_specs": [ms[min(o[t], take_m):min(o[t + 1], take_m)] for t in range(T)],
        }

    def scan_events_tipsets_device(self, receipts_roots, specs, has_ptr: int = 0, cap_receipts: int = 0, matches_ptr: int = 0,
                                   match_spec_ptr: int = 0, cap_matches: int = 0, spec_counts_ptr: int = 0,
                                   receipt_off_ptr: int = 0, match_off_ptr: int = 0):
        """ipcfp_scan_events_tipsets_device: the concatenated map, the records, match_spec, the per-spec counts and (optionally)
        the two offset arrays stay in HBM (pointers of the caller, 0: not wanted).
        → (status u8[T], phase u8[T], receipt_off u64[T+1], match_off u64[T+1], n_receipts, n_matches)"""
        roots = cid_slots(list(receipts_roots)).copy() if len(receipts_roots) else np.zeros((0, CID_SLOT), dtype=np.uint8)
        filt, has_a, actors = self._scan_specs(specs)
        T = len(receipts_roots)
        st = np.zeros(max(T, 1), dtype=np.uint8)
        ph = np.zeros(max(T, 1), dtype=np.uint8)
        roff = np.zeros(T + 1, dtype=np.uint64)
        moff = np.zeros(T + 1, dtype=np.uint64)
        nr, nm = C.c_uint64(), C.c_uint64()
        self.eng._check(self.lib.ipcfp_scan_events_tipsets_device(self.eng.h, self.h, _p(roots), T, _p(filt), _p(has_a), _p(actors),
                                                                  len(specs), _p(st), _p(ph), _p(roff), _p(moff),
                                                                  receipt_off_ptr or None, match_off_ptr or None,
                                                                  has_ptr or None, int(cap_receipts), C.byref(nr),
                                                                  matches_ptr or None, match_spec_ptr or None, int(cap_matches),
                                                                  C.byref(nm), spec_counts_ptr or None), "scan_events_tipsets_device")
        return st[:T].copy(), ph[:T].copy(), roff, moff, int(nr.value), int(nm.value)

    # -- generator side -------------------------------------------------------------------------
    def generate_event_proofs(self, parent_cids, child_cid: bytes, topic0: bytes, topic1: bytes, actor=None):
        """generate_event_proof over this witness as the blockstore.  Returns
        (status, matches structured[n], message_cids u8[n,40], witness block ids u32[m] in `Cid: Ord` order)."""
        pc = pack_cids(parent_cids)
        child = cid_slots([child_cid])[0].copy()
        filt = np.frombuffer(bytes(topic0) + bytes(topic1), dtype=np.uint8).copy()
        st = np.zeros(1, dtype=np.uint8)
        npf, nb = C.c_uint64(), C.c_uint64()
        a = (0, 0) if actor is None else (1, int(actor))
        args = (self.eng.h, self.h, _p(pc), len(parent_cids), _p(child), _p(filt), a[0], a[1], _p(st))
        self.eng._check(self.lib.ipcfp_generate_event_proofs(*args, None, None, 0, C.byref(npf), None, None, 0,
                                                             C.byref(nb)), "generate_event_proofs")
        m = np.zeros(int(npf.value), dtype=MATCH_DTYPE)
        msg = np.zeros((int(npf.value), CID_SLOT), dtype=np.uint8)
        ids = np.zeros(int(nb.value), dtype=np.uint32)
        if st[0] == 1 and (len(m) or len(ids)):
            self.eng._check(self.lib.ipcfp_generate_event_proofs(*args, _p(m), _p(msg), len(m), C.byref(npf), _p(ids),
                                                                 None, len(ids), C.byref(nb)), "generate_event_proofs")
        return int(st[0]), m, msg, ids

    def generate_event_claims(self, parent_cids, child_cid: bytes, topic0: bytes, topic1: bytes, actor=None):
        """generate_event_proof whose proofs stay in HBM as packed claims (ipcfp_generate_event_claims).
        → (status, GeneratedEvents or None when the status is not 1)."""
        pc = pack_cids(parent_cids)
        child = cid_slots([child_cid])[0].copy()
        filt = np.frombuffer(bytes(topic0) + bytes(topic1), dtype=np.uint8).copy()
        st = np.zeros(1, dtype=np.uint8)
        h = C.c_void_p()
        a = (0, 0) if actor is None else (1, int(actor))
        self.eng._check(self.lib.ipcfp_generate_event_claims(self.eng.h, self.h, _p(pc), len(parent_cids), _p(child), _p(filt),
                                                             a[0], a[1], _p(st), C.byref(h)), "generate_event_claims")
        return int(st[0]), (GeneratedEvents(self.eng, h) if h.value else None)

    def generate_event_claims_tipsets(self, pairs, topic0: bytes, topic1: bytes, actor=None) -> "GeneratedEvents":
        """generate_event_claims for a CHAIN of tipset pairs in one pass (ipcfp_generate_event_claims_tipsets).
        pairs: [(parent CIDs, child CID), …] in chain order.  → GeneratedEvents over the whole chain: what the single
        calls give laid end to end, with `tipset_count`, `tipsets`, `tipset_status` and `tipset_claim_off`; a failing
        tipset contributes nothing."""
        off = np.zeros(len(pairs) + 1, dtype=np.uint32)
        for t, (parents, _) in enumerate(pairs):
            off[t + 1] = off[t] + len(parents)
        flat = [c for parents, _ in pairs for c in parents]
        pc = cid_slots(flat) if flat else np.zeros((1, CID_SLOT), dtype=np.uint8)
        children = cid_slots([child for _, child in pairs]) if len(pairs) else np.zeros((1, CID_SLOT), dtype=np.uint8)
        filt = np.frombuffer(bytes(topic0) + bytes(topic1), dtype=np.uint8).copy()
        h = C.c_void_p()
        a = (0, 0) if actor is None else (1, int(actor))
        self.eng._check(self.lib.ipcfp_generate_event_claims_tipsets(self.eng.h, self.h, _p(pc), _p(off), _p(children), len(pairs),
                                                                     _p(filt), a[0], a[1], C.byref(h)), "generate_event_claims_tipsets")
        return GeneratedEvents(self.eng, h)

    def event_claims_from_matches_device(self, matches_ptr: int, n: int, message_cids_ptr: int, parent_epoch: int, child_epoch: int,
                                         tipset: int, claims_out_ptr: int, blob_out_ptr: int, cap_blob: int):
        """ipcfp_event_claims_from_matches_device over device pointers → (rc, blob length).  The return code is handed
        back (not raised): IPCFP_E_INVALID for a short buffer and IPCFP_E_UNSUPPORTED are results a caller branches on."""
        bl = C.c_uint64()
        rc = self.lib.ipcfp_event_claims_from_matches_device(self.eng.h, self.h, matches_ptr or None, n, message_cids_ptr or None,
                                                             parent_epoch, child_epoch, tipset, claims_out_ptr or None,
                                                             blob_out_ptr or None, cap_blob, C.byref(bl))
        return int(rc), int(bl.value)

    def generate_storage_proofs(self, child_cid: bytes, actor_ids, slots32):
        """generate_storage_proof for n (actor_id, slot) specs.  Returns (records GEN_STORAGE_DTYPE[n],
        witness block ids of the union in `Cid: Ord` order)."""
        child = cid_slots([child_cid])[0].copy()
        ids_in = np.ascontiguousarray(actor_ids, dtype=np.uint64)
        slots = np.ascontiguousarray(slots32, dtype=np.uint8).reshape(-1, 32)
        n = len(ids_in)
        out = np.zeros(n, dtype=GEN_STORAGE_DTYPE)
        nb = C.c_uint64()
        wid = np.zeros(max(self.n, 1), dtype=np.uint32)
        self.eng._check(self.lib.ipcfp_generate_storage_proofs(self.eng.h, self.h, _p(child), _p(ids_in), _p(slots), n,
                                                               _p(out), _p(wid), None, len(wid), C.byref(nb)),
                        "generate_storage_proofs")
        return out, wid[: int(nb.value)]

    def generate_storage_claims(self, child_cid: bytes, child_epoch: int, actor_ids, slots32) -> "GeneratedStorageClaims":
        """generate_storage_proof for n (actor_id, slot) specs whose proofs stay in HBM as column claims
        (ipcfp_generate_storage_claims) → GeneratedStorageClaims (a context manager)."""
        child = cid_slots([child_cid])[0].copy()
        ids_in = np.ascontiguousarray(actor_ids, dtype=np.uint64)
        slots = np.ascontiguousarray(slots32, dtype=np.uint8).reshape(-1, 32)
        n = len(ids_in)
        h = C.c_void_p()
        self.eng._check(self.lib.ipcfp_generate_storage_claims(self.eng.h, self.h, _p(child), int(child_epoch), _p(ids_in) if n else None,
                                                               _p(slots) if n else None, n, C.byref(h)), "generate_storage_claims")
        return GeneratedStorageClaims(self.eng, h)

    def generate_storage_claims_device(self, child_cid: bytes, child_epoch: int, actor_ids_ptr: int, slots_ptr: int,
                                       n: int) -> "GeneratedStorageClaims":
        """The same with the specs resident in HBM: actor ids u64[n], slots u8[n][32] on a 16-byte boundary."""
        child = cid_slots([child_cid])[0].copy()
        h = C.c_void_p()
        self.eng._check(self.lib.ipcfp_generate_storage_claims_device(self.eng.h, self.h, _p(child), int(child_epoch),
                                                                      actor_ids_ptr or None, slots_ptr or None, int(n), C.byref(h)),
                        "generate_storage_claims_device")
        return GeneratedStorageClaims(self.eng, h)

    def generate_storage_claims_tipsets(self, child_cids, child_epochs, actor_ids, slots32) -> "GeneratedStorageClaims":
        """The same list of n_specs (actor_id, slot) specs posed at every child of a chain (child_cids: CID bytes per tipset,
        child_epochs: one epoch each) in one pass (ipcfp_generate_storage_claims_tipsets) → GeneratedStorageClaims over
        n_tipsets · n_specs claims in (tipset, spec) order, with `n_tipsets`, `tipset_first_error(t)`, `tipset_block_ids(t)`."""
        children = np.ascontiguousarray(cid_slots(list(child_cids))).reshape(-1, 40) if len(child_cids) else np.zeros((0, 40), np.uint8)
        epochs = np.ascontiguousarray(child_epochs, dtype=np.int64)
        if len(epochs) != len(children):
            raise ValueError("one epoch per child")
        ids_in = np.ascontiguousarray(actor_ids, dtype=np.uint64)
        slots = np.ascontiguousarray(slots32, dtype=np.uint8).reshape(-1, 32)
        n = len(ids_in)
        h = C.c_void_p()
        self.eng._check(self.lib.ipcfp_generate_storage_claims_tipsets(
            self.eng.h, self.h, _p(children) if len(children) else None, _p(epochs) if len(epochs) else None, len(children),
            _p(ids_in) if n else None, _p(slots) if n else None, n, C.byref(h)), "generate_storage_claims_tipsets")
        return GeneratedStorageClaims(self.eng, h)

    def generate_storage_claims_tipsets_device(self, child_cids, child_epochs, actor_ids_ptr: int, slots_ptr: int,
                                               n_specs: int) -> "GeneratedStorageClaims":
        """The same with the spec list resident in HBM: actor ids u64[n_specs], slots u8[n_specs][32] on a 16-byte boundary
        (the children and their epochs stay host arrays)."""
        children = np.ascontiguousarray(cid_slots(list(child_cids))).reshape(-1, 40) if len(child_cids) else np.zeros((0, 40), np.uint8)
        epochs = np.ascontiguousarray(child_epochs, dtype=np.int64)
        if len(epochs) != len(children):
            raise ValueError("one epoch per child")
        h = C.c_void_p()
        self.eng._check(self.lib.ipcfp_generate_storage_claims_tipsets_device(
            self.eng.h, self.h, _p(children) if len(children) else None, _p(epochs) if len(epochs) else None, len(children),
            actor_ids_ptr or None, slots_ptr or None, int(n_specs), C.byref(h)), "generate_storage_claims_tipsets_device")
        return GeneratedStorageClaims(self.eng, h)

    # -- verifiers (claim arrays are ctypes arrays of the ipcfp.h structs) -------------------
    def verify_storage_proofs(self, claims_arr, n, trust=None):
        st = np.zeros(n, dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_verify_storage_proofs(
            self.eng.h, self.h, C.cast(claims_arr, C.c_void_p), n,
            C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None, _p(st)), "verify_storage_proofs")
        return st

    def verify_event_proofs(self, claims_arr, n, trust=None, filt=None):
        st = np.zeros(n, dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_verify_event_proofs(
            self.eng.h, self.h, C.cast(claims_arr, C.c_void_p), n,
            C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            C.cast(C.pointer(filt), C.c_void_p) if filt is not None else None, _p(st)), "verify_event_proofs")
        return st

    # -- one tipset over several GPUs -----------------------------------------------
    def shard_plan_tipset(self, parent_cids, child_cid: bytes, n_shards: int, shard: int):
        """Blocks of this (whole-tipset) witness that `shard` of `n_shards` needs.  Returns
        (status, receipt_lo, receipt_hi, n_receipts, block ids u32[] ascending)."""
        pc = pack_cids(parent_cids)
        child = cid_slots([child_cid])[0].copy()
        st = np.zeros(1, dtype=np.uint8)
        lo, hi, nr, nb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        ids = np.zeros(max(self.n, 1), dtype=np.uint32)
        self.eng._check(self.lib.ipcfp_shard_plan_tipset(self.eng.h, self.h, _p(pc), len(parent_cids), _p(child),
                                                         int(n_shards), int(shard), _p(st), C.byref(lo), C.byref(hi),
                                                         C.byref(nr), _p(ids), len(ids), C.byref(nb)), "shard_plan_tipset")
        return int(st[0]), int(lo.value), int(hi.value), int(nr.value), ids[: int(nb.value)].copy()

    def shard_plan_tipset_all(self, parent_cids, child_cid: bytes, n_shards: int):
        """Every shard's plan in one call.  Returns (status, n_receipts, receipt_bounds u64[G+1], [ids of shard 0, …])."""
        pc = pack_cids(parent_cids)
        child = cid_slots([child_cid])[0].copy()
        st = np.zeros(1, dtype=np.uint8)
        nr, nids = C.c_uint64(), C.c_uint64()
        bounds = np.zeros(n_shards + 1, dtype=np.uint64)
        soff = np.zeros(n_shards + 1, dtype=np.uint64)
        ids = np.zeros(max(self.n, 1) * int(n_shards), dtype=np.uint32)
        self.eng._check(self.lib.ipcfp_shard_plan_tipset_all(self.eng.h, self.h, _p(pc), len(parent_cids), _p(child),
                                                             int(n_shards), _p(st), C.byref(nr), _p(bounds), _p(soff),
                                                             _p(ids), len(ids), C.byref(nids)), "shard_plan_tipset_all")
        lists = [ids[int(soff[s]): int(soff[s + 1])].copy() for s in range(n_shards)]
        return int(st[0]), int(nr.value), bounds, lists

    def subset(self, block_ids, receipt_lo: int = 0, receipt_hi: int = (1 << 64) - 1) -> "Witness":
        """A new witness of the listed blocks (device-side copy), tagged as the receipt-range shard [lo, hi)."""
        ids = np.ascontiguousarray(block_ids, dtype=np.uint32)
        h = C.c_void_p()
        self.eng._check(self.lib.ipcfp_witness_create_subset(self.eng.h, self.h, _p(ids), len(ids), int(receipt_lo),
                                                             int(receipt_hi), C.byref(h)), "witness_create_subset")
        w = Witness.__new__(Witness)
        w.eng, w.lib, w.h, w.n = self.eng, self.lib, h, len(ids)
        return w

    def set_receipt_range(self, lo: int, hi: int):
        self.eng._check(self.lib.ipcfp_witness_set_receipt_range(self.h, int(lo), int(hi)), "set_receipt_range")

    @property
    def receipt_range(self):
        lo, hi = C.c_uint64(), C.c_uint64()
        self.lib.ipcfp_witness_receipt_range(self.h, C.byref(lo), C.byref(hi))
        return int(lo.value), int(hi.value)

    # -- Blockstore face (get / has / put_keyed) ---------------------------------------------------
    def has(self, cids):
        """cids: list[bytes] → (has u8[n], block ids u32[n] with 0xffffffff for absent)."""
        pc = pack_cids(cids)
        has = np.zeros(len(cids), dtype=np.uint8)
        ids = np.zeros(len(cids), dtype=np.uint32)
        self.eng._check(self.lib.ipcfp_witness_has(self.eng.h, self.h, _p(pc), len(cids), _p(has), _p(ids)), "witness_has")
        return has, ids

    def get(self, cid: bytes):
        """Blockstore::get → bytes, or None."""
        c = cid_slots([cid])[0].copy()
        ln, found = C.c_uint64(), C.c_int()
        self.eng._check(self.lib.ipcfp_witness_get(self.eng.h, self.h, _p(c), None, 0, C.byref(ln), C.byref(found)), "witness_get")
        if not found.value:
            return None
        out = np.zeros(max(int(ln.value), 1), dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_witness_get(self.eng.h, self.h, _p(c), _p(out), len(out), C.byref(ln), C.byref(found)), "witness_get")
        return out[: int(ln.value)].tobytes()

    def put_keyed(self, cids, blocks):
        """MemoryBlockstore::put_keyed for a batch: no hashing, an existing CID is replaced."""
        data, off, lens = _table(blocks)
        pc = pack_cids(cids)
        self.eng._check(self.lib.ipcfp_witness_put_keyed(self.eng.h, self.h, _p(pc), _p(data), _p(off), _p(lens), len(cids)),
                        "witness_put_keyed")
        self.n = self.block_count

    def read_values(self, locs: np.ndarray, stride: int = 1024):
        """Bytes of located values (LOC_DTYPE / the block, off, len fields of MATCH_DTYPE) → list[bytes | None]."""
        l = np.zeros(len(locs), dtype=LOC_DTYPE)
        for f in ("block", "off", "len"):
            l[f] = locs[f]
        out = np.zeros((max(len(l), 1), stride), dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_witness_read_values(self.eng.h, self.h, _p(l), len(l), _p(out), stride), "read_values")
        return [None if l["block"][i] == 0xFFFFFFFF else out[i, : min(int(l["len"][i]), stride)].tobytes() for i in range(len(l))]

    def verify_event_proofs_located(self, claims_arr, n, trust=None, filt=None):
        """verify_event_proof + where each proof's StampedEvent lies (for a host check_event closure)."""
        st = np.zeros(n, dtype=np.uint8)
        loc = np.zeros(n, dtype=LOC_DTYPE)
        self.eng._check(self.lib.ipcfp_verify_event_proofs_located(
            self.eng.h, self.h, C.cast(claims_arr, C.c_void_p), n,
            C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            C.cast(C.pointer(filt), C.c_void_p) if filt is not None else None, _p(st), _p(loc)), "verify_event_proofs_located")
        return st, loc

    def verify_event_proofs_with(self, claims_arr, n, check_event, trust=None, filt=None):
        """verify_event_proof with an arbitrary host predicate (events/verifier.rs:51-56,247-251), end to end through
        ipcfp_verify_event_proofs_with: `check_event(proof_index, stamped_event_bytes) -> bool` is called by the
        library, on this thread, for every proof that is otherwise TRUE; False => FALSE_FILTER."""
        st = np.zeros(n, dtype=np.uint8)
        cb_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64)
        raised = []

        def tramp(_user, idx, ptr, ln):
            try:
                return 1 if check_event(int(idx), C.string_at(ptr, int(ln))) else 0
            except BaseException as e:  # a Python exception cannot cross the C frame: keep it, decline, re-raise below
                raised.append(e)
                return 0

        cb = cb_t(tramp)
        self.eng._check(self.lib.ipcfp_verify_event_proofs_with(
            self.eng.h, self.h, C.cast(claims_arr, C.c_void_p), n,
            C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            C.cast(C.pointer(filt), C.c_void_p) if filt is not None else None, C.cast(cb, C.c_void_p), None, _p(st)),
            "verify_event_proofs_with")
        if raised:
            raise raised[0]
        return st

    def generate_proof_bundle(self, parent_cids, child_cid: bytes, storage_specs, event_specs):
        """generate_proof_bundle.  storage_specs: [(actor_id, slot32)], event_specs: [(signature, topic_1, actor|None)].
        → dict(storage GEN_STORAGE_DTYPE[], event_status, matches, message_cids, match_spec, block_ids (Cid order),
               first_error | None)"""
        pc = pack_cids(parent_cids)
        child = cid_slots([child_cid])[0].copy()
        ss = np.zeros(len(storage_specs), dtype=STORAGE_SPEC_DTYPE)
        for i, (a, slot) in enumerate(storage_specs):
            ss["actor_id"][i] = a
            ss["slot"][i] = np.frombuffer(bytes(slot), dtype=np.uint8)
        es = (EventProofSpec * max(len(event_specs), 1))()
        keep = []
        for j, (sig, t1, actor) in enumerate(event_specs):
            keep += [sig.encode(), t1.encode()]
            es[j].event_signature, es[j].topic_1 = keep[-2], keep[-1]
            es[j].has_actor_id_filter = 0 if actor is None else 1
            es[j].actor_id_filter = 0 if actor is None else int(actor)
        sout = np.zeros(max(len(ss), 1), dtype=GEN_STORAGE_DTYPE)
        est = np.zeros(max(len(event_specs), 1), dtype=np.uint8)
        cap_p, cap_b = 1 << 16, max(self.n, 1)
        m = np.zeros(cap_p, dtype=MATCH_DTYPE)
        mc = np.zeros((cap_p, CID_SLOT), dtype=np.uint8)
        ms = np.zeros(cap_p, dtype=np.uint32)
        ids = np.zeros(cap_b, dtype=np.uint32)
        npf, nb, fe = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.eng._check(self.lib.ipcfp_generate_proof_bundle(
            self.eng.h, self.h, _p(pc), len(parent_cids), _p(child), _p(ss), len(ss), C.cast(es, C.c_void_p),
            len(event_specs), _p(sout), _p(est), _p(m), _p(mc), _p(ms), cap_p, C.byref(npf), _p(ids), None, cap_b,
            C.byref(nb), C.byref(fe)), "generate_proof_bundle")
        k = min(int(npf.value), cap_p)
        return {"storage": sout[: len(ss)], "event_status": est[: len(event_specs)], "matches": m[:k], "message_cids": mc[:k],
                "match_spec": ms[:k], "block_ids": ids[: int(nb.value)],
                "first_error": None if fe.value == (1 << 64) - 1 else int(fe.value)}

    def rebuild_index(self):
        """K4 again, in place (no allocation)."""
        self.eng._check(self.lib.ipcfp_witness_rebuild_index(self.eng.h, self.h), "rebuild_index")

    def verify_storage_claims_device(self, claims_ptr: int, n: int, status_ptr: int, trust=None):
        """Packed storage claims resident in HBM (ipcfp_storage_claim_t[n])."""
        self.eng._check(self.lib.ipcfp_verify_storage_claims_device(
            self.eng.h, self.h, claims_ptr, n, C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            status_ptr), "verify_storage_claims_device")

    def verify_storage_claims(self, claims: np.ndarray, trust=None) -> np.ndarray:
        """Packed storage claims in HOST memory: upload + verify + status bytes back (PCIe-inclusive)."""
        claims = np.ascontiguousarray(claims, dtype=SCLAIM_DTYPE)
        st = np.zeros(len(claims), dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_verify_storage_claims(
            self.eng.h, self.h, _p(claims), len(claims), C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            _p(st)), "verify_storage_claims")
        return st

    def verify_storage_columns(self, cols: "StorageColumns", trust=None) -> np.ndarray:
        """The column form in HOST memory (ipcfp_verify_storage_columns): upload, verify, status bytes back."""
        st = np.zeros(cols.n, dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_verify_storage_columns(
            self.eng.h, self.h, cols.h, C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None, _p(st)),
            "verify_storage_columns")
        return st

    def verify_storage_columns_device(self, runs_ptr: int, n_runs: int, slot_ptr: int, value_ptr: int, cflags_ptr: int, n: int,
                                      status_ptr: int, trust=None):
        """The column form resident in HBM (run table n_runs × 192 bytes, slot / value n × 32, cflags n)."""
        self.eng._check(self.lib.ipcfp_verify_storage_columns_device(
            self.eng.h, self.h, runs_ptr or None, int(n_runs), slot_ptr or None, value_ptr or None, cflags_ptr or None, int(n),
            C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None, status_ptr or None), "verify_storage_columns_device")

    def expand_storage_claims_device(self, runs_ptr: int, n_runs: int, slot_ptr: int, value_ptr: int, cflags_ptr: int, n: int,
                                     claims_out_ptr: int):
        """The column form resident in HBM → ipcfp_storage_claim_t[n] at claims_out_ptr (needs no witness: any Witness's engine)."""
        self.eng._check(self.lib.ipcfp_expand_storage_claims_device(
            self.eng.h, runs_ptr or None, int(n_runs), slot_ptr or None, value_ptr or None, cflags_ptr or None, int(n),
            claims_out_ptr or None), "expand_storage_claims_device")

    def verify_event_claims_device(self, tipsets: np.ndarray, claims_ptr: int, n: int, blob_ptr: int, blob_len: int,
                                   status_ptr: int, trust=None, filt=None):
        """Packed claims resident in HBM (ipcfp_event_claim_t[n]); status bytes are written to status_ptr."""
        cached = getattr(self, "_tipset_args", None)
        if cached is None or cached[0] is not tipsets:  # (same array object as last time: its pointer is kept)
            ts = np.ascontiguousarray(tipsets, dtype=TIPSET_DTYPE)
            cached = (tipsets, ts, _p(ts), len(ts))
            self._tipset_args = cached if ts is tipsets else None  # (a converted copy would go stale)
        self.eng._check(self.lib.ipcfp_verify_event_claims_device(
            self.eng.h, self.h, cached[2], cached[3], claims_ptr, n, blob_ptr, blob_len,
            C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            C.cast(C.pointer(filt), C.c_void_p) if filt is not None else None, status_ptr), "verify_event_claims_device")

    def verify_and_scan_device(self, tipsets: np.ndarray, claims_ptr: int, n: int, blob_ptr: int, blob_len: int, status_ptr: int,
                               topic0: bytes, topic1: bytes, actor, has_ptr: int, cap_receipts: int, matches_ptr: int = 0,
                               cap_matches: int = 0, trust=None, filt=None):
        """verify_event_claims_device + scan_events_device of tipsets[0]'s child in ONE call (ipcfp_verify_and_scan_device).
        → (scan status, n_receipts, n_matches); status bytes, has-match map and match records are in the caller's HBM."""
        key = (id(tipsets), bytes(topic0), bytes(topic1))
        cached = getattr(self, "_vs_args", None)
        if cached is None or cached[0] != key:  # (the marshalled arguments of a repeated call are kept)
            ts = np.ascontiguousarray(tipsets, dtype=TIPSET_DTYPE)
            sf = np.frombuffer(bytes(topic0) + bytes(topic1), dtype=np.uint8).copy()
            st = np.zeros(1, dtype=np.uint8)
            nr, nm = C.c_uint64(), C.c_uint64()
            cached = (key, ts, sf, st, nr, nm, _p(ts), len(ts), _p(sf), _p(st), C.byref(nr), C.byref(nm), tipsets)
            self._vs_args = cached
        _, ts, sf, st, nr, nm, p_ts, n_ts, p_sf, p_st, r_nr, r_nm, _keep = cached
        a = (0, 0) if actor is None else (1, int(actor))
        self.eng._check(self.lib.ipcfp_verify_and_scan_device(
            self.eng.h, self.h, p_ts, n_ts, claims_ptr, n, blob_ptr, blob_len,
            C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            C.cast(C.pointer(filt), C.c_void_p) if filt is not None else None, status_ptr, p_sf, a[0], a[1], p_st,
            has_ptr or None, int(cap_receipts), r_nr, matches_ptr or None, int(cap_matches), r_nm), "verify_and_scan_device")
        return int(st[0]), int(nr.value), int(nm.value)

    def verify_event_claims(self, tipsets: np.ndarray, claims: np.ndarray, blob: np.ndarray, blob_len: int,
                            trust=None, filt=None) -> np.ndarray:
        """Packed claims in HOST memory: upload + verify + status bytes back (PCIe-inclusive)."""
        tipsets = np.ascontiguousarray(tipsets, dtype=TIPSET_DTYPE)
        claims = np.ascontiguousarray(claims, dtype=CLAIM_DTYPE)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        st = np.zeros(len(claims), dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_verify_event_claims(
            self.eng.h, self.h, _p(tipsets), len(tipsets), _p(claims), len(claims), _p(blob), blob_len,
            C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            C.cast(C.pointer(filt), C.c_void_p) if filt is not None else None, _p(st)), "verify_event_claims")
        return st

    def verify_event_claims_range(self, tipsets: np.ndarray, claims: np.ndarray, blob: np.ndarray, blob_len: int, lo: int, hi: int,
                                  last: bool, trust=None, filt=None):
        """The claims of the receipts [lo, hi) out of a packed batch in exec_index order (ipcfp_verify_event_claims_range: two
        binary searches, no host pass, offsets rebased on the device).  `last`: the last shard also owns the claims that name
        no receipt.  Returns (first position, status u8[count])."""
        tipsets = np.ascontiguousarray(tipsets, dtype=TIPSET_DTYPE)
        if not (claims.flags.c_contiguous and claims.dtype == CLAIM_DTYPE and blob.flags.c_contiguous):
            raise EngineError("verify_event_claims_range: the batch must be contiguous ipcfp_event_claim_t records")
        st = np.zeros(len(claims), dtype=np.uint8)
        first, count = C.c_uint64(), C.c_uint64()
        self.eng._check(self.lib.ipcfp_verify_event_claims_range(
            self.eng.h, self.h, _p(tipsets), len(tipsets), claims.ctypes.data_as(C.c_void_p), len(claims),
            blob.ctypes.data_as(C.c_void_p), int(blob_len), int(lo), int(hi), int(bool(last)),
            C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            C.cast(C.pointer(filt), C.c_void_p) if filt is not None else None, C.byref(first), C.byref(count), _p(st)),
            "verify_event_claims_range")
        return int(first.value), st[: int(count.value)]

    def verify_event_claims_compact(self, tipsets: np.ndarray, groups: np.ndarray, claims: np.ndarray, cblob: np.ndarray,
                                    cblob_len: int, trust=None, filt=None) -> np.ndarray:
        """Claims in transport form in HOST memory (ipcfp_verify_event_claims_compact): upload, expand on the device,
        verify, status bytes back."""
        tipsets = np.ascontiguousarray(tipsets, dtype=TIPSET_DTYPE)
        groups = np.ascontiguousarray(groups, dtype=GROUP_DTYPE)
        claims = np.ascontiguousarray(claims, dtype=COMPACT_DTYPE)
        cblob = np.ascontiguousarray(cblob, dtype=np.uint8)
        st = np.zeros(len(claims), dtype=np.uint8)
        self.eng._check(self.lib.ipcfp_verify_event_claims_compact(
            self.eng.h, self.h, _p(tipsets), len(tipsets), _p(groups), len(groups), _p(claims), len(claims), _p(cblob), cblob_len,
            C.cast(C.pointer(trust), C.c_void_p) if trust is not None else None,
            C.cast(C.pointer(filt), C.c_void_p) if filt is not None else None, _p(st)), "verify_event_claims_compact")
        return st

    @property
    def cid_bitmap_ptr(self) -> int:
        return int(self.lib.ipcfp_witness_cid_bitmap_device(self.h) or 0)

    @property
    def cid_status_ptr(self) -> int:
        return int(self.lib.ipcfp_witness_cid_status_device(self.h) or 0)
