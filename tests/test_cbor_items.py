"""CPU: the single-item table of tests/cbor_item_cases.py under three judges — the LITERAL verdict written by the rule that
generates each row, tests/pystorage.py `decode` (an independent reader: written from the survey, Python's own UTF-8
decoder) and the C++ oracle — through every carrier; the counting asserts that hold the TABLE (a later edit cannot hollow
it out without notice); and the guard that the limits the sweeps aim at still stand in the engine's source."""
import collections
import os
import re

import pytest

import cbor_item_cases as cc
import pyevents
import pystorage

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ipc-filecoin-proofs_amd", "csrc")
CHECKS = {"any": lambda x: x, "vec_u8": pystorage.check_vec_u8, "receipt": pyevents.check_receipt, "cid": pyevents.check_cid_value,
          "actor_state": pystorage.check_actor_state}
CARRIERS = ("amt_v0", "amt_v3", "hamt")
PER = {"amt_v0": cc.AMT_SHAPE[0][1], "amt_v3": cc.AMT_SHAPE[3][1], "hamt": cc.HAMT_PER_TREE}


def batch_of(carrier, cases, kind, last_block=False):
    if carrier == "hamt":
        return cc.hamt_batch(cases, kind, last_block=last_block)
    return cc.amt_batch(cases, int(carrier[-1]), kind, last_block=last_block)


def judged(block, carrier, kind):
    """the independent judge over one carrier block: it decodes, and every value in it passes the kind's typed check"""
    try:
        tree = pystorage.decode(block)
        values = [e[1] for e in tree[1][0]] if carrier == "hamt" else tree[2]
        for v in values:
            CHECKS[kind](v)
        return True
    except pystorage.Err:
        return False


def oracle_answers(oracle, carrier, b, kind):
    st = oracle.store(*b.store.tables())
    if carrier == "hamt":
        status, values = st.hamt_get(b.root, 5, kind, b.queries, cap=1024)
    else:
        status, values = st.amt_get(b.root, int(carrier[-1]), kind, b.queries, cap=1024)
    st.close()
    return status.tolist(), values


def test_the_judge_gives_every_literal_on_the_bare_item():
    """pystorage.decode over the item alone, row by row: a disagreement is a finding about the judge or about the table"""
    wrong = [(r.group, r.name, r.item[:24].hex()) for r in cc.ROWS if judged_bare(r.item) != r.ok]
    assert not wrong, wrong


def judged_bare(item):
    try:
        pystorage.decode(item)
        return True
    except pystorage.Err:
        return False


@pytest.mark.parametrize("group", cc.ANY_GROUPS + cc.TYPED_KINDS)
def test_judge_and_oracle_give_every_literal_through_every_carrier(oracle, group):
    kind, cases = cc.kind_of(group), cc.cases_of(group)
    wrong, seen = [], collections.Counter()
    for carrier in CARRIERS:
        for part in cc.batches(cases, PER[carrier]):
            b = batch_of(carrier, part, kind)
            status, values = oracle_answers(oracle, carrier, b, kind)
            for c, blk, got, val in zip(part, b.blocks, status, values):
                seen[carrier] += 1
                if judged(blk, carrier, kind) != c.ok:
                    wrong.append((group, c.name, carrier, "pystorage", not c.ok, c.ok))
                if got != (cc.TRUE if c.ok else cc.DECODE) or (c.ok and val != c.item):
                    wrong.append((group, c.name, carrier, "oracle", got, cc.TRUE if c.ok else cc.DECODE))
    assert not wrong, wrong[:20]
    assert all(seen[carrier] == len(cases) for carrier in CARRIERS), seen  # no row is dropped on any carrier


@pytest.mark.parametrize("kind", cc.KINDS)
def test_last_block_variant_judge_and_oracle(oracle, kind):
    """each case in a witness of its own whose LAST block, in the smallest size class of the arena's schedule, is the carrier
    block (cbor_item_cases.amt_batch / hamt_batch assert the layout)"""
    wrong = []
    cases = cc.last_block_cases(kind)
    assert len(cases) >= 40 and {c.ok for c in cases} == {True, False}
    for c in cases:
        for carrier in CARRIERS:
            b = batch_of(carrier, [c], kind, last_block=True)
            status, values = oracle_answers(oracle, carrier, b, kind)
            if judged(b.blocks[0], carrier, kind) != c.ok or status[0] != (cc.TRUE if c.ok else cc.DECODE) or (c.ok and values[0] != c.item):
                wrong.append((c.name, carrier, status[0], c.ok))
    assert not wrong, wrong[:20]


# ---- the header carrier: the whole chain under pystorage / pyevents and the oracle -----------------------------------------------
@pytest.mark.parametrize("long_headers", [False, True])
@pytest.mark.parametrize("which", ["storage", "events"])
def test_header_carrier_judge_and_oracle(oracle, which, long_headers):
    """the item as field 0 / field 15 of a child header: the whole chain under pystorage.verify / pyevents.verify, whose answer
    must be TRUE where the literal says well-formed and ERR_DECODE where not, and the oracle's string verifier"""
    import event_chain_cases as ec
    import storage_chain_cases as sc

    store, claims, names, oks = cc.header_chains(which, long_headers)
    assert len(names) >= 300 and {True, False} == set(oks)
    verify = pystorage.verify if which == "storage" else pyevents.verify
    want = [verify(store.blocks, c) for c in claims]
    wrong = [(n, w, ok) for n, w, ok in zip(names, want, oks) if w != (cc.TRUE if ok else cc.DECODE)]
    assert not wrong, wrong[:20]
    st = oracle.store(*store.tables())
    got = (st.verify_storage_proofs(sc.proofs(claims), mode=1) if which == "storage" else st.verify_event_proofs(ec.proofs(claims), mode=1)).tolist()
    st.close()
    wrong = [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    assert not wrong, wrong[:20]


# ---- the table itself ------------------------------------------------------------------------------------------------------------
def test_counting_the_table():
    by_group = collections.defaultdict(set)
    for r in cc.ROWS:
        by_group[r.group].add(r.ok)
    assert set(by_group) == set(cc.GROUPS) and all(v == {True, False} for v in by_group.values()), by_group  # every group holds both verdicts
    sizes = collections.Counter(r.group for r in cc.ROWS)
    assert sizes["heads"] >= 300 and sizes["utf8"] >= 400 and sizes["major7"] >= 34 and sizes["strings"] >= 50, sizes
    assert sizes["containers"] >= 40 and sizes["tags"] >= 60 and sizes["cids"] >= 24 and len(cc.ROWS) >= 950, sizes
    for kind, rows in cc.TYPED_ROWS.items():
        assert {r.ok for r in rows} == {True, False} and len(rows) >= 90, kind
    # every residue holds both verdicts — in the table's own placement and in the sweep
    table = [c for g in cc.GROUPS for c in cc.cases_of(g)]
    for cases in (table, cc.cases_of("residues"), cc.cases_of("vec_u8")):
        at = collections.defaultdict(set)
        for c in cases:
            if c.at < 16:
                at[c.at].add(c.ok)
        assert set(at) == set(range(16)) and all(v == {True, False} for v in at.values()), at
    # the sweep's subset at all 16 residues and at every offset across the first line's end
    res = cc.cases_of("residues")
    assert len(cc.RESIDUE_ROWS) >= 70 and len(res) == len(cc.RESIDUE_ROWS) * 48
    assert {c.at for c in res} == set(range(16)) | set(range(112, 144)) and {r.ok for r in cc.RESIDUE_ROWS} == {True, False}
    assert {len(r.item) for r in cc.RESIDUE_ROWS} >= {1, 2, 3, 5, 9, 43}
    # the block-end sweep: a prefix of every length 1 to 16, and of every number of bytes cut off 1 to 16
    ends = cc.cases_of("block_end")
    kept, cut = cc.cut_lengths(ends)
    assert set(range(0, 17)) <= kept and set(range(1, 17)) <= cut and set(range(43)) <= kept  # (… and every prefix of a standard link)
    n_ends = sum(1 for r in cc.ROWS if r.ok and len(r.item) <= cc.BLOCK_END_MAX)
    assert n_ends >= 300 and sum(c.name.endswith("+00") for c in ends) == n_ends and not any(c.ok for c in ends)
    # no carrier drops a row: the share of the table a carrier cannot hold is 0 (the longest item fits a leaf of either tree)
    assert max(len(r.item) for r in cc.ROWS) < 1024 - 64
    held = {carrier: sum(len(part) for part in cc.batches(table, PER[carrier])) for carrier in CARRIERS}
    assert all(n == len(cc.ROWS) for n in held.values()), held
    # the header carrier's part of the table
    assert len(cc.HEADER_ROWS) >= 250 and {r.ok for r in cc.HEADER_ROWS} == {True, False}
    assert {f for _, f, *_ in cc.header_cases()} == {0, 15} and any(at > cc.HEADER_STAGE for _, _, at, *_ in cc.header_cases())


def test_the_carriers_place_the_items_where_the_sweeps_say():
    """the residues come out as intended, on every carrier (the builders assert it case by case; here: the whole range is met)"""
    res = cc.cases_of("residues")[:1024]
    for carrier in CARRIERS:
        seen = set()
        for part in cc.batches(res, PER[carrier]):
            b = batch_of(carrier, part, "any")
            for c, blk, o in zip(part, b.blocks, b.offsets):
                assert blk[o:] == c.item and (o % 16 == c.at if c.at < 16 else o == c.at), (carrier, c.name)
                seen.add(o % 128 // 16 if c.at >= 16 else -1 - o % 16)
        assert {-1 - r for r in range(16)} <= seen and {7, 0} <= seen, (carrier, seen)  # … and both sides of the 128-byte line


def _source(*path):
    with open(os.path.join(CSRC, *path), encoding="utf-8") as f:
        return f.read()


def test_limit_guard_the_source_still_states_the_guards_the_sweeps_aim_at():
    """The sweeps aim at the guards of the reader's fast paths and at its four builds; both are read out of the source text.  If
    one moves, this fails and says that the table has to move with it."""
    cbor, body = _source("kernels", "cbor_dev.h"), _source("kernels", "hamt_table_body.h")
    for guard in ("pos + 43u <= n", "at + 48u > r.n", "r.pos + 8u <= r.n", "len <= 8"):
        assert guard in cbor, guard
    assert "e0 + 36u <= r.n" in body
    # the length checks of skip() and head()
    for check in ("a > uint64_t(n - pos)", "a > uint64_t(n - pos) / 2", "nb > n - pos - 1"):
        assert check in cbor, check
    # what the carriers were built around: the standard link's length, the fast entry's key, the items the block-end sweep takes
    assert len(cc.BY_NAME["standard_43_byte_link"].item) == 43 and all(len(k) == 32 for k in cc.hamt_keys()[:4]) and cc.BLOCK_END_MAX >= 43 + 9
    assert len(cc.actor_state(1)) >= 48 and 8 in cc.UTF8_TOTALS and 9 in cc.UTF8_TOTALS
    # the four builds of the reader, in the units the carriers reach
    stage = {unit: re.findall(r"^#define IPCFP_LINE_STAGE (\d)", _source("kernels", unit), re.M)
             for unit in ("cbor_dev.h", "verify_events.hip", "block_events.hip", "hamt_table_lane.hip")}
    assert stage == {"cbor_dev.h": ["0"], "verify_events.hip": ["1"], "block_events.hip": ["1"], "hamt_table_lane.hip": ["2"]}, stage
    assert re.search(r"^#define IPCFP_RD_LDS 1", _source("kernels", "tipset_prepare.hip"), re.M)
    for unit in ("walk.hip", "hamt_levels.hip", "verify_storage.hip", "amt_enum.hip", "amt_dense.hip", "tipset_prepare_general.hip"):
        text = _source("kernels", unit)
        assert "IPCFP_LINE_STAGE" not in text.replace("IPCFP_LINE_STAGE 0", "") and "#define IPCFP_RD_LDS" not in text, unit
    assert re.search(r"kHeaderLds\s*=\s*%d" % cc.HEADER_STAGE, _source("kernels", "tipset_ctx.h") + _source("kernels", "tipset_prologue_body.h")
                     + _source("kernels", "tipset_prepare.hip") + _source("kernels", "tipset_prepare_general.hip"))
