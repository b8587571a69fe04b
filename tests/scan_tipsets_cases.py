"""Chains of tipsets and spec sets for the scan over a CHAIN (ipcfp_scan_events_tipsets), buildable on the CPU.

Every tipset of every chain lives in ONE merged store (as tests/test_gpu_amt_enum_cases.py::merged makes one): a chain is a
list of tipset names, i.e. of receipts roots of that store, and the expected answer of tipset t is
scan_multi_cases.expected(merged blocks, root_t, specs).  The expected phase of a failing tipset is 1 when loading and
enumerating its receipts tree alone raises in pyevents, else 2.

The tipsets come from what the project already holds to account:
    edges, tiles/N, short, err/k      scan_multi_cases (edges, tiles, short_order, err_tipsets)
    rc/NAME                           a receipt case of event_chain_cases.RC alone in a tipset
    ae/NAME                           the receipts tree of a case of amt_enum_cases (sizes, heights, sparse trees, `count` lies)
    own/…                             an undecodable node in a tree of 20, a root no block of the witness carries, tiny trees

A lying `count` is NOT a failure here, although the chains' specification lists it among the RECEIPTS-phase failures:
`Amt::load` reads `count` and nothing compares it (pyevents.AMT_COUNT_IS_NOT_CHECKED, amt_enum_cases "count"), so the oracle,
pyevents and the single-tipset calls all scan such a tree clean.  The chain `count_lies` holds the call to that — sound
tipsets whose plan the lie defeats — and the third RECEIPTS-phase failure beside the absent root and the undecodable node is
a root of height 22 (more than 64 / bit width levels: an Err of the load).

`expected_chain` lays the per-tipset answers end to end: the contract of include/ipcfp.h."""
import functools

import amt_enum_cases as ae
import event_chain_cases as ec
import pyamt
import pyevents
import scan_multi_cases as mc

MAX_TIPSETS = 4096
ABSENT_ROOT = pyamt.cid_of(b"a receipts root no block of the witness carries")
N_TINY = 8

AE_TREES = ("size_0", "size_1", "size_7", "size_8", "size_9", "size_63", "size_64", "size_65", "size_513", "empty_under_height_1",
            "height_3_over_20_receipts", "height_7_over_20_receipts", "height_21_over_20_receipts", "height_22_over_20_receipts",
            "height_25_over_20_receipts", "count_20_receipts_immediate", "count_20_receipts_1_byte_not_minimal",
            "count_says_63_over_64_receipts", "count_says_65_over_64_receipts", "count_says_0_over_64_receipts",
            "count_says_a_million_over_20_receipts_at_height_6", "sparse_single_index_8_pow_2", "sparse_single_index_8_pow_3_minus_1",
            "sparse_one_value_per_leaf_node_1023_nodes")
RC_ALONE = 4  # the first clean and the first failing receipt cases of event_chain_cases.RC, two each


def _tiny(k):
    """tiny tree k: 1 + k % 3 receipts, the first with the usual event (emitter 7000 + k), the rest without events"""
    ev = ec.events_root
    def make(st):
        items = {0: pyamt.receipt(gas=50 + k, events_root=ev(st, {0: ec.good_event(7000 + k)}))}
        for i in range(1, 1 + k % 3):
            items[i] = pyamt.receipt(gas=60 + k + i)
        return pyamt.build_amt(st, items, version=0)
    return make


@functools.lru_cache(maxsize=None)
def world():
    """→ (merged store, {tipset name: receipts root})"""
    store, roots = pyamt.Store(), {}

    def take(blocks):
        for cid, block in blocks.items():
            assert store.blocks.setdefault(cid, block) == block

    est, eparts, _ = mc.edges()
    take(est.blocks)
    roots["edges"] = eparts["receipts"]
    tst, troots = mc.tiles()
    take(tst.blocks)
    for n, r in troots.items():
        roots[f"tiles/{n}"] = r
    sst, sparts = mc.short_order()
    take(sst.blocks)
    roots["short"] = sparts["receipts"]
    for k, (_name, st, parts) in enumerate(mc.err_tipsets()):
        take(st.blocks)
        roots[f"err/{k}"] = parts["receipts"]
    clean, failing = mc.rc_split()
    by_name = {name: mk for name, mk, _cl in ec.RC}
    for name in clean[:RC_ALONE // 2] + failing[-(RC_ALONE // 2):]:
        st, _claim, parts = mc._alone(by_name[name])
        take(st.blocks)
        roots[f"rc/{name}"] = parts["receipts"]
    take(ae.EV_BLOCKS)
    for name in AE_TREES:
        st = pyamt.Store()
        roots[f"ae/{name}"] = ae.CASES[name].receipts(st, {})
        take(st.blocks)
    st = pyamt.Store()
    roots["own/undecodable_node"] = ae.receipts_of({i: ae.R(i) for i in range(20)}, respell={(0, 8): lambda b, l, v: ae.BAD + b"node"})(st, {})
    for k in range(N_TINY):
        roots[f"own/tiny_{k}"] = _tiny(k)(st)
    take(st.blocks)
    roots["own/absent_root"] = ABSENT_ROOT
    assert ABSENT_ROOT not in store.blocks and len(set(roots.values())) == len(roots)
    return store, roots


# ---- spec sets ----------------------------------------------------------------------------------------------------------------------
F0 = (*ec.FILTER, None)            # the usual event: every ae/ and own/tiny tree carries it (emitter 7000 + …), edges some
SPECS_1 = [F0]
SPECS_2 = [F0, (*mc.TILE_ALL, None)]
# one event under several specs (F0 twice and its emitter-filtered twin), a spec that matches in no tipset, pairs of edges
SPECS_8 = [F0, (*ec.FILTER, 7000), (*mc.TILE_ALL, None), (*mc.NOBODY[3], None), (*mc.TILE_PLANTED, 9001), (*mc.pair(0), None), F0, (*mc.pair(0), 8001)]
SPECS_1024 = mc.padded(SPECS_8, 1024)
SPEC_SETS = {"1": SPECS_1, "2": SPECS_2, "8": SPECS_8, "1024": SPECS_1024}


# ---- chains -------------------------------------------------------------------------------------------------------------------------
A, B, C = "ae/size_9", "ae/height_3_over_20_receipts", "short"   # sound; A and B with matches of F0
EMPTY, EMPTY_TALL = "ae/size_0", "ae/empty_under_height_1"
FAIL_RECEIPTS = ("own/absent_root", "own/undecodable_node", "ae/height_22_over_20_receipts")
FAIL_EVENTS = ("err/0", "err/3")
DENSE_POOL = ["ae/size_1", "ae/size_7", "ae/size_8", "ae/size_9", "ae/size_63", "ae/size_64", "ae/size_65", "own/tiny_0", "own/tiny_1",
              "own/tiny_2", "ae/count_20_receipts_immediate"]
TINY_POOL = [f"own/tiny_{k}" for k in range(N_TINY)]


def cycle(pool, n, start=0):
    return [pool[(start + i) % len(pool)] for i in range(n)]


def _chains():
    out = {}

    def chain(name, tipsets, specs="8"):
        assert name not in out
        out[name] = (list(tipsets), specs)

    # T = 1: must equal scan_events_multi byte for byte
    for t in ("edges", "tiles/2049", "err/0", EMPTY, "own/absent_root", "ae/sparse_single_index_8_pow_2"):
        chain(f"one/{t}", [t])
    chain("one/edges/1024_specs", ["edges"], "1024")
    # T = 2: the prefix sum's tile.  Boundaries at 1023, 1024, 1025 and at 2047, 2048, 2049 (the tiles trees plant a second
    # match at receipts 0, 1023, 1024, 2047 and 2048: the last receipt of one tipset and the first of the next both match)
    for a, b in ((1023, 1024), (1023, 1025), (1024, 1024), (1024, 1025), (1025, 1023), (1025, 1024)):
        chain(f"tile/{a}+{b}", [f"tiles/{a}", f"tiles/{b}", "own/tiny_1"])
    chain("tile/1+1023+1024", ["ae/size_1", "tiles/1023", "tiles/1024"], "2")
    # T = 3: a failing tipset of each kind at the first, a middle and the last position, sound tipsets with matches around it
    for f in FAIL_RECEIPTS + FAIL_EVENTS:
        chain(f"fail_first/{f}", [f, A, B])
        chain(f"fail_middle/{f}", [A, f, B])
        chain(f"fail_last/{f}", [A, B, f])
    chain("fail/one_of_each_phase", [A, FAIL_EVENTS[0], B, FAIL_RECEIPTS[0], "edges", FAIL_RECEIPTS[1], A])
    chain("fail/every_tipset", list(FAIL_RECEIPTS + FAIL_EVENTS) + [FAIL_RECEIPTS[0]])
    chain("fail/the_same_failing_root_twice", [FAIL_RECEIPTS[1], A, FAIL_RECEIPTS[1], FAIL_EVENTS[1], FAIL_EVENTS[1]])
    # empty receipts trees
    chain("empty/first", [EMPTY, A, B])
    chain("empty/middle", [A, EMPTY, B])
    chain("empty/last", [A, B, EMPTY])
    chain("empty/two_in_a_row", [A, EMPTY, EMPTY_TALL, B])
    chain("empty/only", [EMPTY, EMPTY_TALL, EMPTY])
    chain("empty/beside_failing", [EMPTY, FAIL_RECEIPTS[0], EMPTY, A, EMPTY, FAIL_EVENTS[0], EMPTY])
    # one root at two positions; two tipsets that share every block but the root
    chain("same_root_twice", [A, "edges", A, "edges"])
    chain("all_blocks_shared_but_the_root", ["ae/count_20_receipts_immediate", "ae/count_20_receipts_1_byte_not_minimal"])
    # trees of different heights side by side, `count` lies, one sparse tree among dense ones
    chain("heights_side_by_side", ["ae/size_1", "ae/size_513", "ae/height_7_over_20_receipts", "ae/size_65", "ae/height_21_over_20_receipts", "ae/size_9"])
    chain("count_lies", ["ae/count_says_63_over_64_receipts", A, "ae/count_says_a_million_over_20_receipts_at_height_6",
                         "ae/count_says_65_over_64_receipts", "ae/count_says_0_over_64_receipts"])
    chain("one_sparse_among_dense", [A, "ae/sparse_single_index_8_pow_3_minus_1", "ae/size_65", "ae/sparse_one_value_per_leaf_node_1023_nodes", A])
    chain("event_chain_cases", [t for t in sorted(world()[1]) if t.startswith("rc/")] + [C])
    # the roots kernel's workgroup (64 / 65) and the dense plan's limit (65 / 66): all dense
    for n in (63, 64, 65, 66):
        chain(f"dense/{n}", cycle(DENSE_POOL, n, start=n))
    chain("dense/64/2_specs", cycle(DENSE_POOL, 64), "2")
    chain("dense/65/1_spec", cycle(DENSE_POOL, 65), "1")
    mixed = cycle(DENSE_POOL + ["ae/sparse_single_index_8_pow_2", EMPTY], 257)
    mixed[0], mixed[100], mixed[101], mixed[256] = FAIL_EVENTS[0], FAIL_RECEIPTS[1], "edges", FAIL_RECEIPTS[0]
    chain("mixed/257", mixed)
    chain("mixed/257/1024_specs", mixed, "1024")
    chain(f"tiny/{MAX_TIPSETS}", cycle(TINY_POOL, MAX_TIPSETS), "2")
    return out


@functools.lru_cache(maxsize=None)
def chains():
    """→ {name: ([tipset name], spec set key)}"""
    return _chains()


def refused_chain():
    """MAX_TIPSETS + 1 tiny tipsets: IPCFP_E_UNSUPPORTED"""
    return cycle(TINY_POOL, MAX_TIPSETS + 1)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def receipts_phase_fails(tipset):
    """loading and enumerating the receipts tree alone raises in pyevents"""
    store, roots = world()
    try:
        list(pyevents.amt_for_each(pyevents.amt_load(store.blocks, roots[tipset], 0, pyevents.check_receipt)))
        return False
    except pyevents.Err:
        return True


@functools.lru_cache(maxsize=None)
def expected_tipset(tipset, specs_key):
    """→ (status, phase, per-spec triples, has map, recorded CIDs) of one tipset: scan_multi_cases.expected over the MERGED blocks"""
    store, roots = world()
    st, per, has, rec = mc.expected(store.blocks, roots[tipset], SPEC_SETS[specs_key])
    if st == pyevents.TRUE:
        assert not receipts_phase_fails(tipset)
        return st, 0, per, has, rec
    return st, 1 if receipts_phase_fails(tipset) else 2, None, None, None


def expected_chain(name):
    """the per-tipset answers laid end to end → dict(status, phase, receipt_off, match_off, has, rows [(exec_index, event_index,
    emitter, spec)], spec_counts, rec (CIDs), maps / records per tipset)"""
    tipsets, key = chains()[name]
    n_specs = len(SPEC_SETS[key])
    out = {"status": [], "phase": [], "receipt_off": [0], "match_off": [0], "has": [], "rows": [], "spec_counts": [0] * n_specs, "rec": set(),
           "maps": [], "records": []}
    for t in tipsets:
        st, phase, per, has, rec = expected_tipset(t, key)
        out["status"].append(st)
        out["phase"].append(phase)
        rows = mc.merge(per) if st == pyevents.TRUE else []
        has = has if st == pyevents.TRUE else []
        out["maps"].append(list(has))
        out["records"].append(rows)
        out["has"] += has
        out["rows"] += rows
        out["receipt_off"].append(len(out["has"]))
        out["match_off"].append(len(out["rows"]))
        if st == pyevents.TRUE:
            out["rec"] |= rec
            for j, p in enumerate(per):
                out["spec_counts"][j] += len(p)
    failing = [p for p in out["phase"] if p]
    out["last_phase"] = failing[0] if failing else 0
    return out


def layout(status, n_idx, n_match, cap_receipts, cap_matches):
    """csrc/host/scan_tipsets_layout.h restated → (receipt_off, match_off, n_receipts, n_matches, map_prefix, match_prefix,
    first_failing)"""
    r_off, m_off, first = [0], [0], -1
    for t, (st, r, m) in enumerate(zip(status, n_idx, n_match)):
        sound = st == pyevents.TRUE
        if not sound and first < 0:
            first = t
        r_off.append(r_off[-1] + (r if sound else 0))
        m_off.append(m_off[-1] + (m if sound else 0))
    return r_off, m_off, r_off[-1], m_off[-1], min(r_off[-1], cap_receipts), min(m_off[-1], cap_matches), first
