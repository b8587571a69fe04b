"""CPU: the AMT enumerator's named cases (tests/amt_enum_cases.py) under two judges — tests/pyevents.py (`amt_for_each`,
`exec_order`, `scan`, `verify`, the first two with the receipt range of a shard) and the C++ oracle (`scan_events`,
`exec_order`, `verify_event_proofs`, `generate_event_proof`) — against the LITERALS written next to each case, and the
assertions that hold the LIST: the limits the cases stand on are the ones csrc/ states, the table has a case below, at and
above each, the plan of the dense walk (tests/native/dense_plan_harness.cpp) says of every case what the case is named
for, every status occurs and every placement of a defect has a claim on and off its path."""
import collections
import os
import re

import numpy as np
import pytest

import amt_enum_cases as ae
import event_chain_cases as ec
import pyevents
import pystorage
from test_dense_plan import DEAD, WHOLE, harness, plan as dense_plan  # noqa: F401  (harness: the fixture)

NAMES = list(ae.CASES)
GROUPS = 16
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ipc-filecoin-proofs_amd", "csrc")
BIG = 10_000  # receipts from which on pyevents walks a whole well-formed tree for a few cases only (3 s each at 65 537)
PY_WHOLE_BIG = {"size_65537", "shared_65537_identical_receipts", "count_65537_receipts_8_byte_not_minimal"}


def n_present(c):
    """receipts the case's scan literal says are delivered"""
    if c.scan[0] != 1:
        return 0
    return c.scan[1] if c.scan[2] == ae.ALL else sum(len(range(*run)) for run in c.scan[2])


def scan_mismatch(c, status, has, triples, where):
    """[] when (status, has-match map, triples) is the case's scan literal"""
    if status != c.scan[0]:
        return [(c.name, where, "scan status", status, c.scan[0])]
    if status != 1:
        return []
    lo = c.rng[0] if c.rng else 0
    present = ae.present_indices(c.scan, c.rng)
    want = np.zeros(c.scan[1], np.uint8)
    want[np.array(present, dtype=np.int64) - lo] = 1
    out = []
    if len(has) != c.scan[1] or not np.array_equal(np.asarray(has, dtype=np.uint8), want):
        out.append((c.name, where, "has-match map", len(has), c.scan[1]))
    if [tuple(int(x) for x in t) for t in triples] != [(i, 0, ae.EMITTER) for i in present]:
        out.append((c.name, where, "triples", len(triples), len(present)))
    return out


def order_mismatch(c, status, cids, where):
    if status != c.order[0]:
        return [(c.name, where, "order status", status, c.order[0])]
    if status != 1:
        return []
    out = []
    if len(cids) != c.order[1]:
        out.append((c.name, where, "order length", len(cids), c.order[1]))
    else:
        out += [(c.name, where, "order position", p) for p, m in c.order[2].items() if bytes(cids[p][:38]) != ae.MSG(m)]
    return out


def claim_mismatch(c, b, got, where):
    return [(c.name, where, tag, int(g), want) for (tag, _cl, want), g in zip(b.claims, got) if int(g) != want]


def generate_literal(c):
    """what generate_event_proof answers, from the case's literals: the execution order's Err, else the scan's, else Err
    (64, "Missing message at index", generator.rs:244-246) when a matching receipt lies behind the last executed message"""
    if c.order[0] != 1:
        return c.order[0]
    if c.scan[0] != 1:
        return c.scan[0]
    present = ae.present_indices(c.scan, None)
    return 64 if present and present[-1] >= c.order[1] else 1


# ---- the two judges --------------------------------------------------------------------------------------------------------------
def pyevents_wrong(c, b):
    name = c.name
    blocks, wrong = b.store.blocks, []
    lo, hi = c.rng if c.rng else (0, None)
    if not (n_present(c) > BIG and name not in PY_WHOLE_BIG):
        st, has, trip, _ = pyevents.scan(blocks, b.parts["receipts"], *ae.FILTER, lo=lo, hi=hi)
        wrong += scan_mismatch(c, st, has, trip, "pyevents")
    big_order = c.order[0] == 1 and c.order[1] > BIG
    try:
        order = exec_order_once(blocks, b) if big_order else pyevents.exec_order(blocks, b.parts["parents"])
        wrong += order_mismatch(c, 1, order, "pyevents")
    except pystorage.Err as e:
        wrong += order_mismatch(c, e.status, None, "pyevents")
    # (verify_event_proof rebuilds the execution order for every claim: for the big lists it gets the one computed above)
    real = pyevents.exec_order
    if big_order:
        pyevents.exec_order = lambda blk, parents, verify_txmeta=True: order
    try:
        wrong += claim_mismatch(c, b, [pyevents.verify(blocks, cl) for _t, cl, _s in b.claims], "pyevents")
    finally:
        pyevents.exec_order = real
    return wrong


_ORDERS = {}


def exec_order_once(blocks, b):
    """pyevents' execution order of a list of more than BIG messages, computed once per set of message lists: every such list
    of the table is a well-formed dense one that many cases share, block for block (the headers and TxMeta above it are
    read by `verify` itself in steps 2 and 3)"""
    key = tuple(b.parts["lists"])
    if key not in _ORDERS:
        _ORDERS[key] = pyevents.exec_order(blocks, b.parts["parents"])
    assert all(p in blocks for p in b.parts["parents"] + b.parts["txmeta"])
    return _ORDERS[key]


def oracle_wrong(oracle, c, b):
    name = c.name
    wrong = []
    ost = oracle.store(*b.store.tables())
    try:
        st, has, trip, touched = ost.scan_events(b.parts["receipts"], *ae.FILTER, cap_receipts=1 << 22, cap_matches=1 << 17)
        if c.rng is None:
            wrong += scan_mismatch(c, st, has, trip, "oracle")
        elif st == 1:  # the oracle has no ranged scan: its whole-tree answer, sliced
            lo, hi = c.rng
            wrong += scan_mismatch(c, 1, has[lo:hi], [t for t in trip if lo <= t[0] < hi], "oracle, sliced")
        # (else: the whole tree fails somewhere; what the range meets of that is pyevents' to say)
        ost_, cids = ost.exec_order(b.parts["parents"], cap=1 << 17)
        wrong += order_mismatch(c, ost_, cids, "oracle")
        if b.claims:
            wrong += claim_mismatch(c, b, ost.verify_event_proofs(ec.proofs([cl for _t, cl, _s in b.claims])), "oracle")
        if c.rng is None and not c.meta.get("shard_witness"):
            gst = ost.generate_event_proof(b.parts["parents"], b.parts["child"], *ae.FILTER, cap_proofs=1 << 17, cap_witness=1 << 17)[0]
            if gst != generate_literal(c):
                wrong.append((name, "oracle", "generate status", gst, generate_literal(c)))
    finally:
        ost.close()
    return wrong


@pytest.mark.parametrize("group", range(GROUPS))
def test_pyevents_the_oracle_and_the_plan_give_every_literal(oracle, harness, group):  # noqa: F811
    """(one test for the three: a case is built once)"""
    wrong = []
    for name in NAMES[group::GROUPS]:
        c, b = ae.CASES[name], ae.build(name)
        wrong += pyevents_wrong(c, b)
        wrong += oracle_wrong(oracle, c, b)
        wrong += plan_wrong(harness, c, b)
    assert not wrong, wrong[:20]


def test_a_ranged_scan_that_fails_is_judged_by_pyevents_alone():
    """… so every such case must exist and pyevents must have been asked (it is: pyevents_wrong skips only status 1)"""
    ranged_err = [n for n, c in ae.CASES.items() if c.rng and c.scan[0] != 1]
    assert len(ranged_err) >= 12 and {ae.CASES[n].scan[0] for n in ranged_err} == {65, 66}


# ---- the cases measure what they are named for ----------------------------------------------------------------------------------
def test_stage_cases_measure_their_leaf():
    seen = set()
    for name, c in ae.CASES.items():
        if "leaf_bytes" not in c.meta:
            continue
        b = ae.build(name)
        if c.meta["leaf_at"] is None:  # the root's node: behind `83 | height | count`
            root = b.store.blocks[b.parts["receipts"]]
            assert root[:3] == bytes([0x83, 0x00, c.meta["n"]])
            got = len(root) - 3
        else:
            got = len(b.store.blocks[b.where[c.meta["leaf_at"]]])
        assert got == c.meta["leaf_bytes"], (name, got)
        seen.add(got)
    edge = ae.STAGE_EDGE
    assert seen == {edge - 1, edge, edge + 1, 512} and edge == 496


def test_shared_trees_are_as_few_blocks_as_they_are_named_for():
    c = ae.CASES["shared_65537_identical_receipts"]
    b = ae.build(c.name)
    tree = {cid for key, cid in b.where.items() if key[0] == "r"} | {b.parts["receipts"]}
    assert len(tree) == c.meta["tree_blocks"] == 11
    b = ae.build("shared_message_list_of_16_equal_leaves")
    assert len({cid for key, cid in b.where.items() if key[0] == "bls0"}) == 2  # one leaf, one node over eight of it


def test_a_shard_witness_holds_no_off_path_block():
    for n in (4097, 65537):
        name = f"range_{n}_on_a_witness_without_the_off_path_blocks"
        b = ae.build(name)
        tree = {cid for key, cid in b.where.items() if key[0] == "r"}
        assert len(tree - set(b.store.blocks)) > len(tree) // 2 and b.parts["receipts"] in b.store.blocks
        # what is left of the tree: the root's paths to [lo, hi) — the leaves 125-374, the height-1 nodes 15-46, the height-2 nodes 1-5, …
        kept = collections.Counter(key[1] for key, cid in b.where.items() if key[0] == "r" and cid in b.store.blocks)
        assert (kept[0], kept[1], kept[2]) == (250, 32, 5), kept


# ---- the list ----------------------------------------------------------------------------------------------------------------------
def test_the_list_covers_what_it_must():
    assert len(NAMES) == len(set(NAMES)) and 450 <= len(NAMES) <= 600
    statuses = collections.Counter(s for c in ae.CASES.values() for _t, _c, s in c.claims)
    statuses.update(c.scan[0] for c in ae.CASES.values())
    statuses.update(c.order[0] for c in ae.CASES.values())
    assert {1, 7, 8, 9, 64, 65, 66} <= set(statuses), statuses
    assert set(ae.FAMILIES) == {"sizes", "heights", "count", "roots", "stage", "links", "shared", "sparse", "two", "ranges"}
    sizes = {c.meta["n"] for c in ae.CASES.values() if c.family == "sizes"}
    assert {0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 32768, 32769, 65472, 65536, 65537, 2040, 2048, 2049} <= sizes
    assert {64 + f for f in range(1, 9)} | {512 + 8 * f for f in range(1, 9)} <= sizes
    heights = {c.meta["height"] for c in ae.CASES.values() if c.family == "heights"}
    assert {0, 1, 2, 3, 8, 9, 10, 20, 21, 22, 23} <= heights
    widths = {(c.meta["width"], c.meta["minimal"]) for c in ae.CASES.values() if "width" in c.meta}
    assert widths == {(0, True), (1, True), (2, True), (4, True), (1, False), (2, False), (4, False), (8, False)}
    assert {c.meta["said"] for c in ae.CASES.values() if "said" in c.meta} == {0, 56, 63, 65, 72, 1_000_000}
    assert {c.meta["parents"] for c in ae.CASES.values() if c.family == "roots"} == {1, 2, 5, 32, 33}
    lengths = {n for c in ae.CASES.values() if c.family == "roots" for pair in c.meta["lengths"] for n in pair}
    assert {0, 1, 8, 9, 64, 65, 513, 4097} <= lengths
    # every placement of a link node's defect has a claim on its path and, below the root, one off it
    for place in ("root", "top", "level", "message_leaf"):
        cs = [c for c in ae.CASES.values() if c.meta.get("place") == place]
        assert len(cs) >= 10 and {c.scan[0] for c in cs} | {c.order[0] for c in cs} >= {1, 65, 66}, place
        assert all(any(t in ("on_the_path", "in_the_hole", "first_of_the_leaf", "any", "the_message_that_stood_there", "the_message_of_the_hole") for t, _c, _s in c.claims) for c in cs), place
        if place in ("top", "level"):
            assert all(any(t in ("off_the_path", "behind_the_hole") and s == 1 for t, _c, s in c.claims) for c in cs), place
    # spelling × placement: every spelling of a link node in the root, in a level of k_dense_top and in one of k_dense_level; of a
    # message-list leaf in the first, the workgroup-ending and the partial last leaf (a leaf of one value has no middle)
    cells = collections.defaultdict(set)
    for c in ae.CASES.values():
        if "place" in c.meta:
            cells[c.meta["place"]].add(c.meta["what"])
            cells[(c.meta["place"], c.meta["pos"])].add(c.meta["what"])
    for place in ("root", "top", "level"):
        assert cells[place] >= ae.INTERIOR_SPELLINGS, (place, ae.INTERIOR_SPELLINGS - cells[place])
    one_link = {"middle_link_of_36_bytes", "last_link_of_36_bytes", "hole"}
    for place, pos in (("top", "first"), ("level", "first"), ("level", "ending_a_workgroup"), ("level", "starting_a_workgroup")):
        assert cells[(place, pos)] >= ae.INTERIOR_SPELLINGS - ({"hole"} if "workgroup" in pos else set()), (place, pos)
    for place in ("top", "level"):
        assert cells[(place, "last_partial")] >= ae.INTERIOR_SPELLINGS - one_link, place
    assert cells["message_leaf"] >= ae.MESSAGE_LEAF_SPELLINGS
    for pos in ("first", "ending_a_workgroup"):
        assert cells[("message_leaf", pos)] >= ae.MESSAGE_LEAF_SPELLINGS, (pos, ae.MESSAGE_LEAF_SPELLINGS - cells[("message_leaf", pos)])
    assert cells[("message_leaf", "last_partial")] >= ae.MESSAGE_LEAF_SPELLINGS - {"first_value_a_36_byte_link", "middle_value_a_36_byte_link"}
    # the receipt heads: the ones the fast check takes, and every one it refuses, in slots 0, 3 and 7
    heads = collections.defaultdict(set)
    for c in ae.CASES.values():
        if "spelled" in c.meta:
            heads[c.meta["spelled"]].add(c.meta["slot"])
            assert c.meta["fast_takes"] == (c.meta["spelled"] in ae.FAST_TAKES)
    assert set(heads) == set(ae.SPELLED) and all(v == {0, 3, 7} for v in heads.values()) and "length_with_an_8_byte_argument" in heads
    assert {c.meta["n"] for c in ae.CASES.values() if "defect" in c.meta} == {513, 4097, 65537}
    # every leaf kernel's family: the receipt leaves (stage), the message leaves, the node-per-lane leaves (the scan of
    # every receipts tree) — a defect on a claimed leaf and beside one
    stage = [c for c in ae.CASES.values() if c.family == "stage" and ("leaf" in c.meta or "spelled" in c.meta)]
    assert {c.scan[0] for c in stage} == {1, 66} and len(stage) >= 40
    assert all({s for _t, _c, s in c.claims} >= {1} for c in stage)
    # two defects: every pair of kinds both ways round
    pairs = {(c.meta["low"], c.meta["high"]) for c in ae.CASES.values() if "low" in c.meta}
    assert pairs == {(a, b) for a in ae.DEFECTS for b in ae.DEFECTS if a != b}
    # ranges: each size, each boundary on and one off either side, and the three defect positions
    for n in (513, 4097, 65537):
        rs = {c.rng for c in ae.CASES.values() if c.family == "ranges" and c.meta["n"] == n and "defect" not in c.meta}
        for B in (8, 64, 512):
            assert {(B, B + 8), (B - 1, B + 8), (B + 1, B + 8), (B - 8, B), (B - 8, B - 1), (B - 8, B + 1)} <= rs, (n, B)
        assert {(n - 5, n), (n - 5, ae.U64), (n + 3, n + 10), (17, 21), (63, 64)} <= rs
    defects = {c.meta["defect"].split("_")[0] for c in ae.CASES.values() if "defect" in c.meta}
    assert defects == {"inside", "first", "last", "off"}


def _source(*path):
    with open(os.path.join(CSRC, *path), encoding="utf-8") as f:
        return f.read()


def _constant(text, name):
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
    assert m, name
    return int(m.group(1))


def limits_in_the_source():
    plan_h, dense, scan, enum_h = _source("kernels", "amt_dense_plan.h"), _source("kernels", "amt_dense.hip"), _source("kernels", "scan.hip"), \
        _source("kernels", "amt_enum.hip")
    top = re.search(r"while \(n_top < (\d+) &&", dense)
    bounds = set(re.findall(r"__launch_bounds__\((\d+)\) void k_dense_\w+", dense))
    small = re.search(r"if \(n <= (\d+)\) \{\s*hipLaunchKernelGGL\(k_scan_small", scan)
    tile = set(re.findall(r"blockIdx\.x \* (\d+)u \+ threadIdx\.x \* 4u", scan)) | set(re.findall(r"div_up\(n, (\d+)\)", scan))
    assert top and small and len(bounds) == 1 and len(tile) == 1 and "launch_scan_u32" in _source("host", "amt_enumerate.cpp") and enum_h
    with open(os.path.join(CSRC, "..", "..", "include", "ipcfp.h"), encoding="utf-8") as f:
        parents = re.search(r"#define IPCFP_MAX_PARENTS (\d+)", f.read())
    return {"dense_top_max": _constant(plan_h, "kDenseTopMax"), "receipt_stage_bytes": _constant(plan_h, "kReceiptStageBytes"),
            "top_levels": int(top.group(1)), "max_dense_levels": _constant(plan_h, "kMaxDenseLevels"), "launch_bound": int(bounds.pop()),
            "general_scan_block": int(tile.pop()), "general_scan_small": int(small.group(1)), "max_parents": int(parents.group(1))}


def test_limit_guard_the_source_still_states_the_limits_the_cases_stand_on():
    """The cases' sizes are literals of tests/amt_enum_cases.py; the engine's constants are read out of its source text.  A
    retuning fails HERE and says which cases have to move."""
    src = limits_in_the_source()
    assert src == ae.LIMITS, {k: (src[k], ae.LIMITS[k]) for k in src if src[k] != ae.LIMITS.get(k)}
    dense = _source("kernels", "amt_dense.hip")
    assert re.search(r"e\.rem <= G \* kReceiptStageBytes - 16u", dense)  # the stage's edge: STAGE_EDGE
    assert "if (n_top >= 2)" in dense
    L = src
    have = collections.defaultdict(set)
    for c in ae.CASES.values():
        for lv in c.meta.get("n_level") or ():
            have["level_entries"].add(lv)
        if "leaf_bytes" in c.meta:
            have["leaf_bytes"].add(c.meta["leaf_bytes"])
        if c.family == "heights" and c.scan[0] == 1:
            have["interior_levels"].add(c.meta["height"])
        if c.family == "heights":
            have["height"].add(c.meta["height"])
        if c.family == "sparse" and c.meta.get("stride") == 8:
            have["general_frontier"].add(c.meta["nodes"])
        if c.family == "roots":
            have["parents"].add(c.meta["parents"])
    edge = 8 * L["receipt_stage_bytes"] - 16
    for key, value in (("level_entries", L["dense_top_max"]), ("level_entries", L["launch_bound"]), ("leaf_bytes", edge),
                       ("interior_levels", L["top_levels"]), ("height", L["max_dense_levels"]), ("general_frontier", L["general_scan_block"]),
                       ("general_frontier", L["general_scan_small"]), ("general_frontier", 5 * L["general_scan_block"])):
        assert {value - 1, value, value + 1} <= have[key], (key, value, sorted(have[key]))
    assert {L["max_parents"], L["max_parents"] + 1} <= have["parents"]


def test_the_entry_points_hand_the_enumerator_amtv0_trees_only():
    """every call site of the enumerator passes version 0 (Amtv0: bit width 3) — the only form the cases build"""
    calls = []
    for path in (("host", "scan_events.cpp"), ("host", "verify_events.cpp")):
        calls += re.findall(r"amt_enumerate_cached\(ctx, w, [\w.]+, (\w+), (\w+),", _source(*path))
    assert calls and all(c == ("0", "VK_RECEIPT") for c in calls), calls
    body = _source("kernels", "tipset_prologue_body.h")
    assert re.search(r"rs\.version = 0;", body) and re.search(r"bls\.version = secp\.version = 0;", body)
    assert set(re.findall(r"\bversion = (\w+);", body)) == {"0"}  # (no other version is ever assigned there)
    assert re.search(r"en->version = 0;", _source("host", "verify_fast.cpp"))
    assert "amt_enumerate(" not in _source("host", "scan_events.cpp")  # (the scan goes through the cache)


# ---- the plan of the dense walk, case by case --------------------------------------------------------------------------------------
def root_info(blocks, cid, check):
    try:
        a = pyevents.amt_load(blocks, cid, 0, check)
    except pystorage.Err:
        return DEAD
    return (a.height, 3, a.count)


def plan_wrong(lib, c, b):
    """the verify call's plan (the message lists whole, the receipts tree as the extra root under the case's range) against the
    case's `plan`; the scan's own plan (the receipts tree alone) against the `n_level` the case is named for"""
    name, blocks, wrong = c.name, b.store.blocks, []
    lists = [root_info(blocks, r, pyevents.check_cid_value) for pair in b.parts["lists"] for r in pair]
    receipts = root_info(blocks, b.parts["receipts"], pyevents.check_receipt)
    rng = c.rng or WHOLE
    if len(lists) + 1 <= lib.max_roots:
        p = dense_plan(lib, lists, want_keys=True, extra=receipts, extra_rng=rng)
        joined = p["ok"] and p["n_use"] == len(lists) + 1
    else:
        joined = False  # more roots than the walk's table holds: the host does not ask
    if c.plan is not None and joined != c.plan:
        wrong.append((name, "verify call's plan", joined, c.plan))
    if receipts != DEAD and c.meta.get("n_level"):
        p = dense_plan(lib, [receipts], rng=rng)
        if not p["ok"] or p["n_level"][: len(c.meta["n_level"])] != c.meta["n_level"]:
            wrong.append((name, "n_level", p["n_level"][:8], c.meta["n_level"]))
    return wrong


def test_every_case_states_its_plan():
    assert all(c.plan is not None for c in ae.CASES.values())
    assert sum(1 for c in ae.CASES.values() if not c.plan) >= 30 and sum(1 for c in ae.CASES.values() if c.meta.get("n_level")) >= 16


def test_the_seams_of_the_dense_walk_are_where_the_cases_say(harness):  # noqa: F811
    """k_dense_top takes the levels of at most kDenseTopMax entries, at most 8 of them; k_dense_level the rest"""
    top = harness.top_max
    assert top == ae.LIMITS["dense_top_max"]
    for n, in_top in ((65472, [1023, 128, 16, 2]), (65536, [1024, 128, 16, 2]), (65537, [129, 17, 3])):
        lv = ae.CASES[f"size_{n}"].meta["n_level"]
        taken, level = [], len(lv) - 1
        while len(taken) < 8 and level >= 1 and lv[level - 1] <= top:
            taken.append(lv[level - 1])
            level -= 1
        assert sorted(taken) == sorted(in_top), (n, taken)
    # the link-node cases: 8200 receipts — heights 4, 3, 2 in the top launch, height 1 by k_dense_level
    p = dense_plan(harness, [(4, 3, ae.LN)])
    assert p["ok"] and p["n_level"][:5] == [1025, 129, 17, 3, 1]


# ---- tests/pyamt.py writes the bytes it always wrote -------------------------------------------------------------------------------
PINNED_ROOTS = {
    "dense_600_receipts": ("0171a0e402207cb54eea8cc8fa1a3ff515a0094af7667ecae489f61c099c5f9ab4d6b7d6117b", 88),
    "sparse_mix": ("0171a0e402203afd4f3502bc0ff1e770fd2cce4dc0a203f385bb29ea4d1fc7585172e397230d", 16),
    "sparse_v3_bit_width_5": ("0171a0e402204385fe1e64361058d32bc0cd546903231064861840c1f9ef1b5a4e81748d3086", 11),
    "v3_bit_width_1": ("0171a0e40220389bece457a5d65ea638c6034fa89d8f9e00b5885fb5d2ad2652ef8442122666", 12),
    "height_lies_low": ("0171a0e40220c77f88d1f383f1ec9fd79897e6fe6fdb85459b65c95b02fca94110565bce37b1", 9),
    "height_lies_high_count_lies": ("0171a0e40220cb4dc1b7fc6828675d53b85dc01b1b4b22e17455b07b63db70ce07f8b87d765f", 6),
    "odd_links": ("0171a0e4022038853ffa511ca76719add83af3d27e7007f1716969ed07d2df6f70cf35a0a64c", 88),
    "empty_tall": ("0171a0e40220125c49160b198c3ebf35979cde6b7d6cc3211a5c306c834f51faf1c02d6d7509", 1),
}


def pinned_trees():
    import pyamt
    r = pyamt.receipt
    yield "dense_600_receipts", dict(items={i: r(gas=i) for i in range(600)})
    yield "sparse_mix", dict(items={i: r(gas=i) for i in (0, 5, 64, 65, 4095, 100000)})
    yield "sparse_v3_bit_width_5", dict(items={i: pyamt.uint(i) for i in (3, 31, 32, 1023, 1024, 99999)}, version=3, bit_width=5)
    yield "v3_bit_width_1", dict(items={i: pyamt.uint(i) for i in range(11)}, version=3, bit_width=1)
    yield "height_lies_low", dict(items={i: r(gas=i) for i in range(100)}, height=1)
    yield "height_lies_high_count_lies", dict(items={i: r(gas=i) for i in range(20)}, height=3, count=7)
    yield "odd_links", dict(items={i: r(gas=i) for i in range(600)}, odd_links={(0, 264), (1, 128)})
    yield "empty_tall", dict(items={}, height=2)


def test_pyamt_writes_the_bytes_it_always_wrote():
    """the root CIDs (and with them every block below) of a few trees, pinned from the writer as it was before `_node` sliced its
    sorted items: sparse ones, heights that lie both ways, 36-byte links, bit widths 1 and 5"""
    import pyamt
    got = {}
    for name, kw in pinned_trees():
        st = pyamt.Store()
        got[name] = (pyamt.build_amt(st, kw.pop("items"), **kw).hex(), len(st.blocks))
    assert got == PINNED_ROOTS
