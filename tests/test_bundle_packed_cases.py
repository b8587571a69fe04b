"""CPU: the case table of the packed bundle writer (tests/bundle_packed_cases.py) is consistent, and the engine's HOST route —
ipcfp_unpack_storage_claims of the expanded columns, ipcfp_unpack_event_claims, ipcfp_bundle_write_claims_json — agrees with
the table's Python expectation on every case: the text of the sound ones, (rc, index) of the refused ones.  No device.  The
new entry points are exported and declared in every binding."""
import os
import re

import pytest

import bundle_packed_cases as cases
import ipc_filecoin_proofs_amd as ipcfp
from ipc_filecoin_proofs_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_route(case):
    """→ the head's text, or (rc, kind, index)"""
    rows = cases.expand_rows(case)
    if rows is None:
        return (cases.E_INVALID, cases.STORAGE, None)
    try:
        us = binding.unpack_storage_claims(rows)
    except ipcfp.EngineError as e:
        return (e.rc, cases.STORAGE, e.bad_index)
    with us:
        try:
            ue = binding.unpack_event_claims(case.tipsets, case.claims, case.blob)
        except ipcfp.EngineError as e:
            return (e.rc, cases.EVENTS, e.bad_index)
        with ue:
            return binding.bundle_claims_json(us.ptr or None, us.n, ue.ptr or None, ue.n)


@pytest.mark.parametrize("case", cases.ALL, ids=lambda c: c.name)
def test_host_route_agrees_with_the_table(case):
    assert host_route(case) == case.expected()


def test_merged_sound_cases_agree():
    m = cases.merge(cases.SOUND)
    assert m.n_storage == sum(c.n_storage for c in cases.SOUND) and m.n_events == sum(c.n_events for c in cases.SOUND)
    assert host_route(m) == m.head()


def test_table_covers_what_it_lists():
    by = {c.name: c for c in cases.ALL}
    ints = by["integers"]
    assert {p["parent_epoch"] for p in ints.event_dicts} == set(cases.EPOCHS) == {p["child_epoch"] for p in ints.event_dicts}
    for f in ("exec_index", "event_index", "emitter"):
        assert {p[f] for p in ints.event_dicts} == set(cases.UINTS), f
    assert {p["actor_id"] for p in ints.storage_dicts} == set(cases.UINTS)
    assert {p["child_epoch"] for p in ints.storage_dicts} == set(cases.EPOCHS)
    want = {cases._cidstr(c) for c in cases.SOUND_CIDS}
    cids = by["cids"]
    for f in ("child_block_cid", "parent_state_root", "actor_state_cid", "storage_root"):
        assert {p[f] for p in cids.storage_dicts} == want, f
    assert {p["message_cid"] for p in cids.event_dicts} == want == {p["child_block_cid"] for p in cids.event_dicts}
    assert {s for p in cids.event_dicts for s in p["parent_tipset_cids"]} == want
    shapes = by["event_shapes"]
    assert [(len(p["data"]) - 2) // 2 for p in shapes.event_dicts] == cases.DATA_LENS
    assert {len(p["topics"]) for p in shapes.event_dicts} == set(cases.TOPIC_COUNTS)
    assert {len(p["parent_tipset_cids"]) for p in by["tipsets"].event_dicts} == {1, 5, 32, 33}
    assert [int(n) for n in by["run_lengths"].runs["n_claims"]] == [1, 2, 63, 64, 65, 256, 257]
    pl = cases.placement(cases.SOUND)
    assert all(len(s) == 16 and len(e) == 16 for s, e in pl.values())


def test_new_entry_points_are_declared_everywhere():
    lib = ipcfp.load_library()
    rust_sys = open(os.path.join(ROOT, "bindings", "rust", "ffi_sys.rs")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "ipcfp.h")).read()
    for name in ("ipcfp_bundle_write_packed_json", "ipcfp_bundle_write_generated_json"):
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        assert "pub fn %s(" % name in rust_sys, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "ipcfp_bundle_write_generated_json(" in rust
    assert "#define IPCFP_ABI_VERSION 3" in header and "IPCFP_K_CLAIM_TEXT = 27" in header and "IPCFP_K_COUNT = 28" in header
    assert binding.KERNEL_IDS["claim_text"] == 27 and binding.KERNEL_IDS["gen_tipsets"] == 26
    assert hasattr(ipcfp.Engine, "bundle_write_packed_json") and hasattr(ipcfp.Engine, "bundle_write_generated_json")
