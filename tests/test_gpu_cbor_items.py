"""GPU: the single-item table of tests/cbor_item_cases.py through every carrier and every route of the engine, against the
LITERAL verdict of each row — TRUE with the item's own bytes located, or ERR_DECODE — and, for the header carrier, against
tests/pystorage.py / tests/pyevents.py over the whole witness.

    amt      ipcfp_amt_get, Amtv0 and v3, one case per leaf, several hundred leaves per call
    hamt     ipcfp_hamt_get through the routes of tests/test_gpu_hamt_routes.py and the default, 1024 cases per call
    typed    the same with kind vec_u8 / receipt / cid / actor_state
    header   the event verifier through the routes of tests/test_gpu_event_chain.py `answers`, ipcfp_verify_storage_proofs
             and the packed forms through those of tests/test_gpu_storage_chain.py `answers`
    last     a part of the block-end sweep once more, each case in a witness of its own whose last block is the carrier

The carrier → kernel → reader-build table is the docstring of tests/cbor_item_cases.py.  Measured on an MI355X: the whole
file takes 5 s; the slowest tests are the event verifier over the headers under the stage (0.34 s for the first piece, which
builds the chains; 0.17 s for the others), the storage verifier over them (0.25 s) and the last-block variant of kind `any`
(0.17 s per half: 82 witnesses of one case each, nine calls per witness); no AMT or HAMT piece of 2048 cases takes more than
0.03 s."""
import numpy as np
import pytest

import cbor_item_cases as cc
import pyevents
import pystorage
from test_gpu_hamt_routes import ROUTES, loc_bytes, routed  # noqa: F401 (`routed` is the fixture that restores the tuning)

pytestmark = pytest.mark.gpu

HAMT_ROUTES = ROUTES + [("default", {"hamt_levels": -1, "hamt_table": -1})]
AMT_VERSIONS = (0, 3)


def wrong_in(tag, cases, b, gs, gl, data, off):
    """the cases whose status is not the literal's, or whose located bytes are not the item's"""
    got = loc_bytes(data, off, gl)
    out = []
    for c, s, g, want, val in zip(cases, gs, got, b.want, b.values):
        if int(s) != want:
            out.append((c.group, c.name, tag, int(s), want))
        elif want == cc.TRUE and g != val:
            out.append((c.group, c.name, tag, "located", g[:16].hex(), val[:16].hex()))
    return out[:8]


def through_amt(engine, cases, kind, last_block=False):
    wrong, n = [], 0
    for version in AMT_VERSIONS:
        for part in cc.batches(cases, 1 if last_block else cc.AMT_SHAPE[version][1]):
            b = cc.amt_batch(part, version, kind, last_block=last_block)
            data, off, lens, cids = b.store.tables()
            with engine.witness(data, off, lens, cids) as w:
                gs, gl = w.amt_get(b.root, version, kind, np.array(b.queries, dtype=np.uint64))
            wrong += wrong_in(f"amt_v{version}", part, b, gs, gl, data, off)
            n += len(part)
    assert n == len(AMT_VERSIONS) * len(cases)  # no row is dropped
    return wrong


def through_hamt(engine, routed, cases, kind, last_block=False):
    wrong, n = [], 0
    for part in cc.batches(cases, 1 if last_block else cc.HAMT_PER_TREE):
        b = cc.hamt_batch(part, kind, last_block=last_block)
        data, off, lens, cids = b.store.tables()
        with engine.witness(data, off, lens, cids) as w:
            for route, cfg in HAMT_ROUTES:
                routed(cfg)
                gs, gl = w.hamt_get(b.root, 5, kind, b.queries)
                wrong += wrong_in(f"hamt/{route}", part, b, gs, gl, data, off)
        n += len(part)
    assert n == len(cases)
    return wrong


def parts_of(group):
    """a group in pieces of at most 2048 cases: [(group, piece)]"""
    return [(group, k) for k in range(-(-len(cc.cases_of(group)) // 2048))]


PIECES = [p for g in cc.ANY_GROUPS + cc.TYPED_KINDS for p in parts_of(g)]


@pytest.mark.parametrize("group,piece", PIECES, ids=[f"{g}-{k}" for g, k in PIECES])
def test_amt_leaf_values_every_row(engine, group, piece):
    wrong = through_amt(engine, cc.cases_of(group)[piece * 2048: (piece + 1) * 2048], cc.kind_of(group))
    assert not wrong, wrong[:20]


@pytest.mark.parametrize("group,piece", PIECES, ids=[f"{g}-{k}" for g, k in PIECES])
def test_hamt_bucket_values_every_row_every_route(engine, routed, group, piece):
    wrong = through_hamt(engine, routed, cc.cases_of(group)[piece * 2048: (piece + 1) * 2048], cc.kind_of(group))
    assert not wrong, wrong[:20]


LAST = [(kind, k) for kind in cc.KINDS for k in range(2)]


@pytest.mark.parametrize("kind,half", LAST, ids=[f"{k}-{h}" for k, h in LAST])
def test_carrier_block_last_in_the_arena(engine, routed, kind, half):
    """a witness per case: the carrier block is the last one of the arena's schedule, behind it only the arena's tail"""
    cases = cc.last_block_cases(kind)[half::2]
    wrong = through_amt(engine, cases, kind, last_block=True) + through_hamt(engine, routed, cases, kind, last_block=True)
    assert not wrong, wrong[:20]


# ---- the header carrier ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_headers", [False, True], ids=["under_the_stage", "over_the_stage"])
def test_header_fields_storage_verifier_every_route(engine, routed, long_headers):
    from test_gpu_storage_chain import answers, wrong_answers

    store, claims, names, oks = cc.header_chains("storage", long_headers)
    want = [pystorage.verify(store.blocks, c) for c in claims]
    assert want == [cc.TRUE if ok else cc.DECODE for ok in oks]

    def use(table):
        engine.set_tuning("hamt_table", table)

    with engine.witness(*store.tables()) as w:
        wrong = wrong_answers(answers(w, use, claims), names, want)
    assert not wrong, wrong[:20]


EVENT_BATCH = 96
EVENT_PIECES = [(lh, k) for lh in (False, True) for k in range(4)]


@pytest.mark.parametrize("long_headers,piece", EVENT_PIECES, ids=[f"{'over' if lh else 'under'}_the_stage-{k}" for lh, k in EVENT_PIECES])
def test_header_fields_event_verifier_every_route(engine, long_headers, piece):
    """under the stage the tipset prologue parses the header out of LDS (tipset_prepare.hip), over it the general reader does
    (tipset_prepare_general.hip): the engine chooses by the longest block of the witness, so each has a witness of its own"""
    from test_gpu_event_chain import answers, wrong_answers

    store, claims, names, oks = cc.header_chains("events", long_headers)
    want = [pyevents.verify(store.blocks, c) for c in claims]
    assert want == [cc.TRUE if ok else cc.DECODE for ok in oks]

    def use(fast):
        engine.set_tuning("fast_verify", fast)

    wrong = []
    try:
        with engine.witness(*store.tables()) as w:
            for lo in range(piece * EVENT_BATCH, len(claims), 4 * EVENT_BATCH):
                got = answers(w, use, store.blocks, claims[lo: lo + EVENT_BATCH])
                wrong += wrong_answers(got, names[lo: lo + EVENT_BATCH], want[lo: lo + EVENT_BATCH])
    finally:
        engine.set_tuning("fast_verify", -1)
    assert not wrong, wrong[:20]
