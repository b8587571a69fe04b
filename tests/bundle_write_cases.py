"""Shared by the bundle writer's tests (test_bundle_write_host.py, test_gpu_bundle_write.py): sample claims, their ctypes
arrays, and the expected head of the text by serde_json's escaping rule — json.dumps(ensure_ascii=False, separators=(",", ":"));
the default ensure_ascii=True of bundle_ref's writer escapes 0x7f and everything above, which serde_json copies verbatim."""
import json

import bundle_ref

STORAGE_FIELDS = ("child_epoch", "child_block_cid", "parent_state_root", "actor_id", "actor_state_cid", "storage_root", "slot",
                  "value")


def dump(v) -> str:
    return json.dumps(v, ensure_ascii=False, separators=(",", ":"))


def head_text(storage, events) -> bytes:
    """serde_json::to_string of the two claim vectors (declaration order, serde_json's escapes) + the opening of `blocks`"""
    s = [dump({k: p[k] for k in STORAGE_FIELDS}) for p in storage]
    e = [dump({"parent_epoch": p["parent_epoch"], "child_epoch": p["child_epoch"], "parent_tipset_cids": p["parent_tipset_cids"],
               "child_block_cid": p["child_block_cid"], "message_cid": p["message_cid"], "exec_index": p["exec_index"],
               "event_index": p["event_index"],
               "event_data": {"emitter": p["emitter"], "topics": p["topics"], "data": p["data"]}}) for p in events]
    return ('{"storage_proofs":[%s],"event_proofs":[%s],"blocks":[' % (",".join(s), ",".join(e))).encode("utf-8")


def storage_proof(**kw):
    p = dict(child_epoch=7, child_block_cid="bafy-child", parent_state_root="bafy-root", actor_id=1001,
             actor_state_cid="bafy-actor", storage_root="bafy-storage", slot="0x" + "00" * 32, value="0x" + "11" * 32)
    p.update(kw)
    return p


def event_proof(**kw):
    p = dict(parent_epoch=6, child_epoch=7, parent_tipset_cids=["bafy-p0", "bafy-p1"], child_block_cid="bafy-child",
             message_cid="bafy-msg", exec_index=3, event_index=1, emitter=1234, topics=["0x" + "aa" * 32, "0x" + "bb" * 32],
             data="0x0102")
    p.update(kw)
    return p


def arrays(storage, events):
    ev, st = bundle_ref.claims_from_parsed({"storage_proofs": storage, "event_proofs": events})
    return st, ev
