"""Hand-built trees for the AMT ENUMERATOR (`Amt::for_each` behind reconstruct_execution_order, src/proofs/events/utils.rs:76-90,
and behind the receipt list of find_matching_events, generator.rs:195-204): one NAMED case per limit of the engine's three
routes — the root loader, the dense walk, the general walk (csrc/host/amt_enumerate.cpp) — with its answers written down as
LITERALS:

    CASES[name].scan    (status,) or (1, number of receipts, present) — `present`: ALL, or [(first, stop, step)] index runs
    CASES[name].order   (status,) or (1, length, {position: message number})
    CASES[name].claims  [(tag, {"e": exec_index, "msg": message number | CID, …claim fields}, status)]
    CASES[name].rng     None or the receipt range [lo, hi) the scan and the verifier run under

The literals come from the reference's text and from the named assumptions of tests/pyevents.py; tests/test_amt_enum_cases.py
holds pyevents and the C++ oracle to every one of them, tests/test_gpu_amt_enum_cases.py every entry point of the engine.

Every tree is an Amtv0 (bit width 3): the only form the public entry points hand to the enumerator.  Every receipt names
ONE shared events root with one event that matches FILTER, so that the scan's has-match map says which receipts the
enumeration delivered: has[i] == 1 exactly for the receipts that are present.

A case is BUILT on demand (`build(name)`): the big message lists and receipt trees are cached by size and copied."""
import collections
import functools
import hashlib

import event_chain_cases as ec
import pyamt
from pyamt import array, bstr, link, raw_node, uint

FILTER = ec.FILTER
EMITTER = 7000
EVENT = ec.good_event(EMITTER)
_EV = pyamt.Store()
EV_ROOT = ec.events_root(_EV, {0: EVENT})
EV_SHA = _EV.put(_EV.blocks[EV_ROOT], sha256_cid=True)  # the same events root under a 36-byte sha2-256 CID
EV_BLOCKS = dict(_EV.blocks)
LOG = ec.log_fields(EVENT)
ALL = "all"
U64 = (1 << 64) - 1
BAD = ec.BAD
OTHER = ec.OTHER
GRAND, OLDER, CHILD_MSGS = pyamt.cid_of(b"grandparent header"), pyamt.cid_of(b"older receipts"), pyamt.cid_of(b"child messages")

# ---- the engine's limits the cases stand on (tests/test_amt_enum_cases.py reads them out of csrc/ and compares) -----------------
LIMITS = {"dense_top_max": 1024, "receipt_stage_bytes": 64, "top_levels": 8, "max_dense_levels": 24, "launch_bound": 256,
          "general_scan_block": 1024, "general_scan_small": 4096, "max_parents": 32}
STAGE_EDGE = 8 * LIMITS["receipt_stage_bytes"] - 16  # a group of 8 lanes stages a leaf of up to 496 bytes


@functools.lru_cache(maxsize=None)
def MSG(i) -> bytes:
    return pyamt.cid_of(b"enumerated message %d" % i)


def R(i, ret=b"", root=EV_ROOT):
    return pyamt.receipt(gas=1000 + i, ret=ret, events_root=root)


SAME = pyamt.receipt(gas=1000, events_root=EV_ROOT)  # the receipt of the trees whose equal leaves are one block
RECEIPT_3 = array([uint(0), bstr(b""), uint(1000)])
RECEIPT_5 = array([uint(0), bstr(b""), uint(1000), link(EV_ROOT), uint(0)])


class Case:
    __slots__ = ("name", "family", "receipts", "lists", "scan", "order", "claims", "rng", "plan", "walks", "drop", "meta")


class Built:
    __slots__ = ("store", "parts", "claims", "where")


CASES = collections.OrderedDict()


def case(name, family, *, receipts, lists, scan, order, claims=(), rng=None, plan=None, walks=None, drop=None, **meta):
    """receipts: callable(store, where) → root CID;  lists: callable(store, where) → [(bls root, secp root)] per parent;
    plan: what dense_plan says of the verify call's roots (message lists whole, the receipts tree under `rng`);
    walks: 1 where the packed verify call queues the table route's dense walk on first contact (None: not stated);
    drop: callable(where, parts) → CIDs deleted from the finished store"""
    assert name not in CASES, name
    c = Case()
    c.name, c.family, c.receipts, c.lists, c.scan, c.order, c.claims = name, family, receipts, lists, scan, order, list(claims)
    c.rng, c.plan, c.walks, c.drop, c.meta = rng, plan, walks, drop, meta
    CASES[name] = c
    return c


def claim_of(parts, e, msg, **over):
    m = MSG(msg) if isinstance(msg, int) else msg
    c = {"parent_epoch": ec.PARENT_EPOCH, "child_epoch": ec.CHILD_EPOCH, "parent_tipset_cids": [ec.cid_str(p) for p in parts["parents"]],
         "child_block_cid": ec.cid_str(parts["child"]), "message_cid": ec.cid_str(m), "exec_index": e, "event_index": 0, **LOG}
    c.update(over)
    return c


def build(name) -> Built:
    c = CASES[name]
    st = pyamt.Store()
    st.blocks.update(EV_BLOCKS)
    where = {}
    lists = c.lists(st, where)
    rroot = c.receipts(st, where)
    salt = int.from_bytes(hashlib.sha256(name.encode()).digest()[:3], "big")
    parts = {"parents": [], "txmeta": [], "receipts": rroot, "lists": lists}
    for k, (bls, secp) in enumerate(lists):
        tx = st.put(array([link(bls), link(secp)]))
        parts["txmeta"].append(tx)
        parts["parents"].append(st.put(array(ec.header_fields([GRAND], ec.PARENT_EPOCH, OLDER, tx, salt + k))))
    parts["child"] = st.put(array(ec.header_fields(parts["parents"], ec.CHILD_EPOCH, rroot, CHILD_MSGS, salt + 100)))
    for cid in (c.drop(where, parts) if c.drop else ()):
        del st.blocks[cid]
    b = Built()
    b.store, b.parts, b.where = st, parts, where
    b.claims = [(tag, claim_of(parts, **spec), status) for tag, spec, status in c.claims]
    return b


def present_indices(scan, rng=None):
    """the literal's `present` as a sorted list of absolute indices"""
    _, n, present = scan
    lo = rng[0] if rng else 0
    if present == ALL:
        return list(range(lo, lo + n))
    return [i for first, stop, step in present for i in range(first, stop, step)]


# ---- trees -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _dense_receipts(n):
    st, where = pyamt.Store(), {}
    root = pyamt.build_amt(st, {i: R(i) for i in range(n)}, version=0, where=where)
    return st.blocks, root, {("r",) + k: v for k, v in where.items()}


@functools.lru_cache(maxsize=8)
def _dense_messages(n):
    st = pyamt.Store()
    return st.blocks, pyamt.build_amt(st, {i: link(MSG(i)) for i in range(n)}, version=0)


def receipts_dense(n):
    def make(st, where):
        blocks, root, wh = _dense_receipts(n)
        st.blocks.update(blocks)
        where.update(wh)
        return root
    return make


def receipts_of(items, **kw):
    """items: {index: receipt bytes} or callable() → that;  kw: build_amt's (height, count, odd_links, respell, trailer)"""
    def make(st, where):
        wh = {}
        root = pyamt.build_amt(st, items() if callable(items) else items, version=0, where=wh, **kw)
        where.update({("r",) + k: v for k, v in wh.items()})
        return root
    return make


def message_list(st, numbers, where=None, tag="m", **kw):
    wh = {}
    root = pyamt.build_amt(st, numbers if isinstance(numbers, dict) else {i: link(MSG(m)) for i, m in enumerate(numbers)}, version=0, where=wh, **kw)
    if where is not None:
        where.update({(tag,) + k: v for k, v in wh.items()})
    return root


def one_parent(n, **kw):
    """one parent block: n messages (numbers 0..n-1) in its BLS list, an empty secp list"""
    def make(st, where):
        if kw:
            bls = message_list(st, range(n), where, **kw)
        else:
            blocks, bls = _dense_messages(n)
            st.blocks.update(blocks)
        return [(bls, message_list(st, []))]
    return make


def parents_of(rows, **spelled):
    """rows: [([bls message numbers], [secp message numbers])];  spelled: {"bls0": build_amt kw, …} or a callable per list"""
    def make(st, where):
        out = []
        for k, (bls, secp) in enumerate(rows):
            pair = []
            for which, numbers in (("bls", bls), ("secp", secp)):
                kw = spelled.get(f"{which}{k}", {})
                pair.append(kw(st, where) if callable(kw) else message_list(st, numbers, where, tag=f"{which}{k}", **kw))
            out.append(tuple(pair))
        return out
    return make


def at(i, **over):
    return {"e": i, "msg": i, **over}


def usual_claims(n):
    """the honest claim at the first and the last receipt, a message nobody executed, the first message under the index of
    the second, and an event index no AMT holds (pyevents.AMT_MAX_INDEX_IS_U64_MAX_MINUS_1)"""
    if n == 0:
        return [("nothing_executed", {"e": 0, "msg": OTHER}, 7)]
    out = [("first", at(0), 1), ("last", at(n - 1), 1), ("not_executed", {"e": n, "msg": OTHER}, 7), ("event_index_u64_max", at(0, event_index=U64), 64)]
    if n > 1:
        out.append(("index_of_another", {"e": 1, "msg": 0}, 8))
    return out


# ===== sizes: dense trees 0..n-1, receipts and messages alike =================================================================
# n_level: nodes per level of ONE such tree, leaves first (what the plan of a whole scan must say)
N_LEVEL = {2040: [255, 32, 4, 1], 2048: [256, 32, 4, 1], 2049: [257, 33, 5, 1], 65472: [8184, 1023, 128, 16, 2, 1],
           65536: [8192, 1024, 128, 16, 2, 1], 65537: [8193, 1025, 129, 17, 3, 1], 32768: [4096, 512, 64, 8, 1], 32769: [4097, 513, 65, 9, 2, 1],
           4096: [512, 64, 8, 1], 4097: [513, 65, 9, 2, 1], 512: [64, 8, 1], 513: [65, 9, 2, 1], 8: [1], 9: [2, 1], 64: [8, 1], 65: [9, 2, 1]}
SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2040, 2048, 2049, 4095, 4096, 4097, 32768, 32769, 65472, 65536, 65537)
for _n in SIZES:
    case(f"size_{_n}", "sizes", receipts=receipts_dense(_n), lists=one_parent(_n), scan=(1, _n, ALL),
         order=(1, _n, {0: 0, _n - 1: _n - 1} if _n else {}), claims=usual_claims(_n), plan=True, walks=1 if _n else 0,
         n=_n, n_level=N_LEVEL.get(_n))
# a last leaf and a last interior node of every fill 1..8
for _f in range(1, 9):
    case(f"fill_last_leaf_{_f}", "sizes", receipts=receipts_dense(64 + _f), lists=one_parent(64 + _f), scan=(1, 64 + _f, ALL),
         order=(1, 64 + _f, {0: 0, 63 + _f: 63 + _f}), claims=usual_claims(64 + _f), plan=True, walks=1, n=64 + _f)
    case(f"fill_last_interior_{_f}", "sizes", receipts=receipts_dense(512 + 8 * _f), lists=one_parent(512 + 8 * _f), scan=(1, 512 + 8 * _f, ALL),
         order=(1, 512 + 8 * _f, {0: 0, 511 + 8 * _f: 511 + 8 * _f}), claims=usual_claims(512 + 8 * _f), plan=True, walks=1, n=512 + 8 * _f)

# ===== non-minimal heights =====================================================================================================
# MAX_HEIGHT is 64 / bit width = 21 (pyevents.AMT_MAX_HEIGHT_IS_64_OVER_BIT_WIDTH; assumption_cases.EVENT_CASES holds it for
# widths 5 and 8, "receipts_root_height_*" for width 3): 21 loads, 22 and above is an Err of the load.  Heights 8, 9 and 10
# cross the 8 levels one k_dense_top launch joins; 23, 24 and 25 straddle kMaxDenseLevels.
HEIGHTS = (3, 7, 8, 9, 10, 20, 21, 22, 23, 24, 25)
for _h in HEIGHTS:
    _ok = _h <= 21
    for _n in (20, 600):
        case(f"height_{_h}_over_{_n}_receipts", "heights", receipts=receipts_of({i: R(i) for i in range(_n)}, height=_h), lists=one_parent(_n),
             scan=(1, _n, ALL) if _ok else (66,), order=(1, _n, {0: 0, _n - 1: _n - 1}),
             claims=[("first", at(0), 1 if _ok else 66), ("last", at(_n - 1), 1 if _ok else 66), ("not_executed", {"e": _n, "msg": OTHER}, 7)],
             plan=_ok, walks=1 if _ok else 0, height=_h, n=_n)
    case(f"height_{_h}_over_a_message_list_of_20", "heights", receipts=receipts_dense(20), lists=one_parent(20, height=_h),
         scan=(1, 20, ALL), order=(1, 20, {0: 0, 19: 19}) if _ok else (66,),
         claims=[("first", at(0), 1 if _ok else 66), ("last", at(19), 1 if _ok else 66)], plan=_ok, walks=1 if _ok else 0, height=_h, n=20)
for _h in (0, 1, 2):
    case(f"empty_under_height_{_h}", "heights", receipts=receipts_of({}, height=_h), lists=parents_of([([], [])], bls0={"height": _h}),
         scan=(1, 0, ALL), order=(1, 0, {}), claims=[("nothing_executed", {"e": 0, "msg": OTHER}, 7)], plan=_h == 0, walks=0, height=_h, n=0)

# ===== `count`: every CBOR width, minimal and not; lies ==========================================================================
# `Amt::load` reads `count` as any u64 and nothing compares it (pyevents.AMT_COUNT_IS_NOT_CHECKED); serde_ipld_dagcbor takes
# an integer in a wider head than it needs (event_chain_cases "receipts_count_spelled_in_two_bytes")
def _width(n, extra):
    return bytes([0x18 + (0, 1, 2, 4, 8).index(extra) - 1]) + n.to_bytes(extra, "big") if extra else bytes([n])


COUNT_WIDTHS = {20: (0, 1, 2, 4, 8), 200: (1, 2, 4, 8), 600: (2, 4, 8), 65537: (4, 8)}  # the first of each is the minimal one
for _n, _ws in COUNT_WIDTHS.items():
    for _w in _ws:
        _tag = ("immediate" if _w == 0 else f"{_w}_byte") + ("" if _w == _ws[0] else "_not_minimal")
        case(f"count_{_n}_receipts_{_tag}", "count", receipts=receipts_of((lambda n: lambda: {i: R(i) for i in range(n)})(_n), count=_width(_n, _w)),
             lists=one_parent(_n), scan=(1, _n, ALL), order=(1, _n, {0: 0, _n - 1: _n - 1}), claims=usual_claims(_n), plan=True, walks=1,
             n=_n, width=_w, minimal=_w == _ws[0])
        if _n != 65537:
            case(f"count_{_n}_messages_{_tag}", "count", receipts=receipts_dense(_n), lists=one_parent(_n, count=_width(_n, _w)),
                 scan=(1, _n, ALL), order=(1, _n, {0: 0, _n - 1: _n - 1}), claims=usual_claims(_n), plan=True, walks=1, n=_n, width=_w,
                 minimal=_w == _ws[0])
# lies around a node boundary: 64 values (8 full leaves under one root)
for _said, _plan in ((63, True), (65, False), (56, True), (72, False), (0, False)):
    # (65 and 72 are more than a root of height 1 can hold: no dense candidate; 0 under a height: likewise)
    case(f"count_says_{_said}_over_64_receipts", "count", receipts=receipts_of({i: R(i) for i in range(64)}, count=_said), lists=one_parent(64),
         scan=(1, 64, ALL), order=(1, 64, {0: 0, 63: 63}), claims=usual_claims(64), plan=_plan, n=64, said=_said)
    case(f"count_says_{_said}_over_64_messages", "count", receipts=receipts_dense(64), lists=one_parent(64, count=_said),
         scan=(1, 64, ALL), order=(1, 64, {0: 0, 63: 63}), claims=usual_claims(64), plan=_plan, n=64, said=_said)
case("count_says_a_million_over_20_receipts_at_height_6", "count", receipts=receipts_of({i: R(i) for i in range(20)}, height=6, count=1_000_000),
     lists=one_parent(20), scan=(1, 20, ALL), order=(1, 20, {0: 0, 19: 19}), claims=usual_claims(20), plan=True, walks=1, n=20, said=1_000_000)
case("count_says_a_million_over_20_messages_at_height_6", "count", receipts=receipts_dense(20), lists=one_parent(20, height=6, count=1_000_000),
     scan=(1, 20, ALL), order=(1, 20, {0: 0, 19: 19}), claims=usual_claims(20), plan=True, walks=1, n=20, said=1_000_000)

# ===== several roots side by side ================================================================================================
def seq(first, n):
    return list(range(first, first + n))


def _roots(name, rows, n_distinct, positions, claims, receipts=None, scan=None, plan=True, walks=1, **kw):
    """receipts: as many as there are distinct messages unless given"""
    case(name, "roots", receipts=receipts or receipts_dense(n_distinct), lists=parents_of(rows, **kw.pop("spelled", {})),
         scan=scan or (1, n_distinct, ALL), order=(1, n_distinct, positions), claims=claims, plan=plan, walks=walks, parents=len(rows),
         lengths=[(len(b), len(s)) for b, s in rows], **kw)


# one parent; message 2 once more at slot 5 of the BLS list → 513 + 9 - 1 distinct
_r = seq(0, 513)
_r[5] = 2
_roots("roots_1_parent_513_and_9_duplicate_within_the_list", [(_r, seq(513, 9))], 521, {0: 0, 4: 4, 5: 6, 6: 7, 511: 512, 512: 513, 520: 521},
       [("first", at(0), 1), ("the_duplicate_at_its_first_place", {"e": 2, "msg": 2}, 1), ("the_duplicate_at_its_second_place", {"e": 5, "msg": 2}, 8),
        ("behind_the_duplicate", {"e": 5, "msg": 6}, 1), ("last", {"e": 520, "msg": 521}, 1), ("raw_position_of_the_last", {"e": 521, "msg": 521}, 8)])
# two parents, the tallest first; the second's secp list starts with the first message of its BLS list
_roots("roots_2_parents_tallest_first_duplicate_across_bls_and_secp", [(seq(0, 4097), []), (seq(5000, 8), [5000] + seq(6000, 64))], 4169,
       {0: 0, 4096: 4096, 4097: 5000, 4104: 5007, 4105: 6000, 4168: 6063},
       [("first", at(0), 1), ("last_of_the_tall_list", at(4096), 1), ("the_duplicate_at_its_first_place", {"e": 4097, "msg": 5000}, 1),
        ("the_duplicate_at_its_second_place", {"e": 4105, "msg": 5000}, 8), ("behind_the_duplicate", {"e": 4105, "msg": 6000}, 1),
        ("last", {"e": 4168, "msg": 6063}, 1)])
# five parents, the tallest in the middle, empty lists between tall ones; the last parent repeats the first one's first message
_roots("roots_5_parents_tallest_in_the_middle_duplicate_across_parents",
       [(seq(0, 64), [100]), ([], seq(1000, 513)), (seq(2000, 4097), []), ([], []), ([0] + seq(7000, 512), seq(8000, 9))], 5196,
       {0: 0, 63: 63, 64: 100, 65: 1000, 577: 1512, 578: 2000, 4674: 6096, 4675: 7000, 5186: 7511, 5187: 8000, 5195: 8008},
       [("first", at(0), 1), ("the_duplicate_where_the_last_parent_has_it", {"e": 4675, "msg": 0}, 8), ("behind_the_duplicate", {"e": 4675, "msg": 7000}, 1),
        ("last_of_the_tallest", {"e": 4674, "msg": 6096}, 1), ("last", {"e": 5195, "msg": 8008}, 1)])
# 32 parents (IPCFP_MAX_PARENTS: 64 message roots and the receipts root are kMaxDenseRoots), the tallest last:
# parent k < 31 has 8 (k even) or 1 (k odd) BLS messages and 9 secp messages when 3 divides k — 16·8 + 15·1 + 11·9 = 242
_rows32, _next = [], 0
for _k in range(31):
    _b = seq(_next, 8 if _k % 2 == 0 else 1)
    _next += len(_b)
    _s = seq(_next, 9 if _k % 3 == 0 else 0)
    _next += len(_s)
    _rows32.append((_b, _s))
_rows32.append((seq(10000, 4097), seq(20000, 65)))
_roots("roots_32_parents_tallest_last", _rows32, 4404, {0: 0, 7: 7, 8: 8, 241: 241, 242: 10000, 4338: 14096, 4339: 20000, 4403: 20064},
       [("first", at(0), 1), ("last_of_the_short_parents", at(241), 1), ("first_of_the_tallest", {"e": 242, "msg": 10000}, 1),
        ("last", {"e": 4403, "msg": 20064}, 1), ("not_executed", {"e": 4404, "msg": OTHER}, 7)])
# 33 parents: one more than the dense walk's root table holds; the last parent's secp message is the first parent's first
_rows33 = [(seq(0, 65), [900])] + [(seq(1000 + 10 * k, 8), [1008 + 10 * k]) for k in range(31)] + [(seq(1310, 8), [0])]
_roots("roots_33_parents_duplicate_across_the_first_and_the_last", _rows33, 353, {0: 0, 64: 64, 65: 900, 66: 1000, 344: 1308, 345: 1310, 352: 1317},
       [("first", at(0), 1), ("the_duplicate_in_the_last_parent", {"e": 353, "msg": 0}, 8), ("last", {"e": 352, "msg": 1317}, 1)], plan=False, walks=0)
# the anomaly may be the extra root's: a hole in the receipts tree beside dense lists — and the other way round
_roots("roots_receipts_with_a_hole_beside_dense_lists", [(seq(0, 4097), []), (seq(5000, 8), seq(6000, 65))], 4170, {0: 0, 4169: 6064},
       [("first", at(0), 1), ("in_the_hole", at(3), 9), ("behind_the_hole", at(4), 1), ("last", {"e": 4169, "msg": 6064}, 1)],
       receipts=receipts_of({i: R(i) for i in range(4170) if i != 3}, count=4170), scan=(1, 4170, [(0, 3, 1), (4, 4170, 1)]))
_roots("roots_a_list_with_a_hole_beside_a_dense_receipts_tree", [(seq(0, 513), seq(600, 9)), (seq(700, 65), [])], 586, {0: 0, 2: 2, 3: 4, 511: 512, 512: 600, 585: 764},
       [("first", at(0), 1), ("behind_the_hole", {"e": 3, "msg": 4}, 1), ("the_message_of_the_hole", {"e": 3, "msg": 3}, 7), ("last", {"e": 585, "msg": 764}, 1)],
       receipts=receipts_dense(587), scan=(1, 587, ALL),
       spelled={"bls0": lambda st, where: message_list(st, {i: link(MSG(i)) for i in range(513) if i != 3}, where, tag="bls0", count=513)})

# ===== receipt leaves around the stage of k_dense_receipt_leaves ================================================================
# 20 receipts: leaves of 8, 8 and 4 values; a plain receipt here is 49 bytes, a full plain leaf 5 + 8 · 49 = 397
def _ret_for(leaf_bytes, values_in_leaf):
    """the return-data length that makes a leaf of `values_in_leaf` receipts, one of them long, exactly `leaf_bytes` long"""
    plain = 5 + 49 * values_in_leaf
    for n in range(1, 1000):
        if plain - 1 + len(bstr(bytes(n))) == leaf_bytes:
            return n
    raise AssertionError(leaf_bytes)


def _stage(name, slot, leaf_bytes, n=20, **kw):
    """the long receipt at index `slot`; the case MEASURES its leaf (meta leaf_bytes is compared with the block's length)"""
    in_leaf = min(8, n - (slot & ~7))
    ret = bytes(_ret_for(leaf_bytes, in_leaf))
    case(name, "stage", receipts=receipts_of({i: R(i, ret=ret if i == slot else b"") for i in range(n)}), lists=one_parent(n),
         scan=(1, n, ALL), order=(1, n, {0: 0, n - 1: n - 1}), claims=usual_claims(n) + [("the_long_one", at(slot), 1)], plan=True, walks=1,
         leaf_bytes=leaf_bytes, leaf_at=("r", 0, slot & ~7) if n > 8 else None, n=n, **kw)


for _bytes in (STAGE_EDGE - 1, STAGE_EDGE, STAGE_EDGE + 1, 512):
    _stage(f"stage_leaf_of_{_bytes}_bytes_long_receipt_in_slot_0", 8, _bytes)
    _stage(f"stage_leaf_of_{_bytes}_bytes_long_receipt_in_slot_7", 15, _bytes)
    _stage(f"stage_leaf_of_{_bytes}_bytes_long_receipt_in_the_partial_last_leaf", 18, _bytes)
    _stage(f"stage_root_leaf_of_{_bytes}_bytes", 3, _bytes, n=8)  # (the leaf is the root's node: it starts behind the root's heads)

# receipt heads around the fast value check (receipt_value_fast), beside plain neighbours: the wider heads it still TAKES (an exit
# code or a length of up to four argument bytes, gas of any width) and every one it refuses and leaves to the reader
def _spelled_receipt(i, what):
    gas, lk = uint(1000 + i), link(EV_ROOT)
    return {"exit_code_in_a_wider_head": array([b"\x18\x00", bstr(b""), gas, lk]),
            "length_in_a_wider_head": array([uint(0), b"\x58\x00", gas, lk]),
            "gas_in_a_wider_head": array([uint(0), bstr(b""), b"\x1b" + (1000 + i).to_bytes(8, "big"), lk]),
            "length_with_an_8_byte_argument": array([uint(0), b"\x5b" + (3).to_bytes(8, "big") + b"abc", gas, lk]),
            "exit_code_with_an_8_byte_argument": array([b"\x1b" + (7).to_bytes(8, "big"), bstr(b""), gas, lk]),
            "exit_code_2_pow_32": array([b"\x1b" + (1 << 32).to_bytes(8, "big"), bstr(b""), gas, lk]),
            "events_root_a_36_byte_sha256_link": array([uint(0), bstr(b""), gas, link(EV_SHA)]),
            "events_root_a_byte_string": array([uint(0), bstr(b""), gas, bstr(b"\x00" + EV_ROOT)]),
            "a_3_tuple": RECEIPT_3, "a_5_tuple": RECEIPT_5}[what]


# what the reference makes of each: a wider head is the same number; 2^32 does not fit `exit_code: u32`; a byte string is no Cid
FAST_TAKES = ("exit_code_in_a_wider_head", "length_in_a_wider_head", "gas_in_a_wider_head")  # (the others: refused, the reader decides)
SPELLED = {"exit_code_in_a_wider_head": 1, "length_in_a_wider_head": 1, "gas_in_a_wider_head": 1, "exit_code_with_an_8_byte_argument": 1,
           "length_with_an_8_byte_argument": 1,
           "exit_code_2_pow_32": 66, "events_root_a_36_byte_sha256_link": 1, "events_root_a_byte_string": 66, "a_3_tuple": 66, "a_5_tuple": 66}
for _what, _st in SPELLED.items():
    for _slot in (0, 3, 7):
        _i = 8 + _slot  # in the middle leaf of three
        case(f"receipt_{_what}_in_slot_{_slot}", "stage", receipts=receipts_of({i: _spelled_receipt(i, _what) if i == _i else R(i) for i in range(20)}),
             lists=one_parent(20), scan=(1, 20, ALL) if _st == 1 else (_st,), order=(1, 20, {0: 0, 19: 19}),
             claims=[("the_spelled_one", at(_i), _st), ("its_neighbour_in_the_leaf", at(_i ^ 1), _st), ("in_another_leaf", at(1), 1)],
             plan=True, walks=1, n=20, spelled=_what, slot=_slot, fast_takes=_what in FAST_TAKES)


def _respelled_leaf(base, fn, n=20, tree="r"):
    return receipts_of({i: R(i) for i in range(n)}, respell={(0, base): fn})


LEAF_SPELLINGS = {  # name: (callable(bitmap, links, values) → node bytes, status of the scan and of a claim on the leaf)
    "one_trailing_byte_after_its_last_value": (lambda b, l, v: raw_node(b, l, v, trailer=b"\x00"), 66),
    "values_array_head_in_the_two_byte_form": (lambda b, l, v: raw_node(b, l, v, values_head=b"\x98" + bytes([len(v)])), 1),
    "a_link_in_front_of_its_values": (lambda b, l, v: raw_node(b, [link(OTHER)], v), 66),
    "bitmap_one_byte_long": (lambda b, l, v: raw_node(b + b"\x00", l, v), 66),
    "bitmap_empty": (lambda b, l, v: raw_node(b"", l, v), 66),
    "one_value_more_than_bits": (lambda b, l, v: raw_node(bytes([b[0] >> 1]), l, v), 66),
    "one_value_fewer_than_bits": (lambda b, l, v: raw_node(b, l, v[:-1]), 66),
}
for _what, (_fn, _st) in LEAF_SPELLINGS.items():
    for _pos, _base in (("first", 0), ("middle", 8), ("last_partial", 16)):
        case(f"receipt_leaf_{_pos}_with_{_what}", "stage", receipts=_respelled_leaf(_base, _fn), lists=one_parent(20),
             scan=(1, 20, ALL) if _st == 1 else (_st,), order=(1, 20, {0: 0, 19: 19}),
             claims=[("on_the_leaf", at(_base + 1), _st), ("on_another_leaf", at((_base + 8) % 24 + 1), 1)], plan=True, walks=1, n=20, leaf=_what, pos=_pos)

# ===== link nodes ==================================================================================================================
# 8200 receipts: 1025 leaves, 129 nodes at height 1, 17 at 2, 3 at 3, the root at 4.  The dense walk takes heights 4, 3 and 2
# in k_dense_top (3, 17 and 129 children) and height 1 in k_dense_level (1025 children: more than kDenseTopMax); the
# children of the height-1 nodes 31 and 32 are lanes 248-255 and 256-263 of that launch: the workgroup boundary.
LN = 8200
ML = 2049  # messages of the message-leaf cases below: 257 leaves, the last one partial
LINKS_IN = {(4, 0): 3, (2, 0): 8, (2, 8192): 1, (1, 0): 8, (1, 31 * 64): 8, (1, 32 * 64): 8, (1, 8192): 1}  # links of the nodes below
LINK_NODE_AT = {  # placement: (node height, [(position, node base, an index under it — under the respelled link where one is, an index under no defect)])
    "root": (4, [("root", 0, 0, None)]),
    "top": (2, [("first", 0, 0, 5000), ("last_partial", 8192, 8192, 5000)]),
    "level": (1, [("first", 0, 0, 5000), ("ending_a_workgroup", 31 * 64, 31 * 64, 5000), ("starting_a_workgroup", 32 * 64, 32 * 64, 5000),
                  ("last_partial", 8192, 8192, 5000)]),
}


def _two_byte_link(lk):
    assert lk[:4] == b"\xd8\x2a\x58\x27"
    return b"\xd8\x2a\x59\x00\x27" + lk[4:]


# name: (callable(bitmap, links, values) → node bytes, status of the whole scan, status of a claim under link 0 of the node)
LINK_SPELLINGS = {
    "bitmap_one_byte_long": (lambda b, l, v: raw_node(b + b"\x00", l, v), 66, 66),
    "bitmap_one_byte_short": (lambda b, l, v: raw_node(b"", l, v), 66, 66),  # (bit width 3: one byte, so none)
    "one_link_more_than_bits": (lambda b, l, v: raw_node(b, l + [link(OTHER)], v), 66, 66),
    "one_link_fewer_than_bits": (lambda b, l, v: raw_node(b, l[:-1] if len(l) > 1 else [], v) if len(l) > 1 else raw_node(bytes([b[0] | 2]), l, v), 66, 66),
    "first_link_with_a_two_byte_length_head": (lambda b, l, v: raw_node(b, [_two_byte_link(l[0])] + l[1:], v), 1, 1),
    "last_link_with_a_two_byte_length_head": (lambda b, l, v: raw_node(b, l[:-1] + [_two_byte_link(l[-1])], v), 1, 1),
    "a_value_behind_the_links": (lambda b, l, v: raw_node(b, l, [R(0)]), 66, 66),
    "a_trailing_byte": (lambda b, l, v: raw_node(b, l, v, trailer=b"\x00"), 66, 66),
}
for _place, (_h, _where) in LINK_NODE_AT.items():
    for _pos, _base, _on, _off in _where:
        _tag = f"{_place}_{_pos}" if _place != "root" else "root"
        for _what, (_fn, _scan, _claim) in LINK_SPELLINGS.items():
            _kw = {"trailer": b"\x00"} if (_place, _what) == ("root", "a_trailing_byte") else {"respell": {(_h, _base): _fn}}
            case(f"link_node_{_tag}_{_what}", "links", receipts=receipts_of((lambda: {i: R(i) for i in range(LN)}), **_kw), lists=one_parent(LN),
                 scan=(1, LN, ALL) if _scan == 1 else (_scan,), order=(1, LN, {0: 0, LN - 1: LN - 1}),
                 claims=[("on_the_path", at(_on), _claim)] + ([("off_the_path", at(_off), 1)] if _off is not None else []),
                 plan=not (_place == "root" and _scan != 1), walks=0 if _place == "root" and _scan != 1 else 1,  # (a root that does not load)
                 place=_place, pos=_pos, what=_what, n=LN)
        # a 36-byte link first, in the middle and last; a hole; a missing target: by the child's place
        _span = 8 ** _h
        _first_child = (_h - 1, _base)
        _m = LINKS_IN[(_h, _base)]
        for _which, _k in (("first", 0), ("middle", _m // 2), ("last", _m - 1)):
            if _k == 0 and _which != "first":
                continue  # (a node of one link: its first link is its last)
            case(f"link_node_{_tag}_{_which}_link_of_36_bytes", "links",
                 receipts=receipts_of((lambda: {i: R(i) for i in range(LN)}), odd_links={(_h - 1, _base + _k * _span)}),
                 lists=one_parent(LN), scan=(1, LN, ALL), order=(1, LN, {0: 0, LN - 1: LN - 1}),
                 claims=[("on_the_path", at(_base + _k * _span), 1)] + ([("off_the_path", at(_off), 1)] if _off is not None else []), plan=True, walks=1,
                 place=_place, pos=_pos, what=f"{_which}_link_of_36_bytes", n=LN)
        case(f"link_node_{_tag}_first_target_missing", "links", receipts=receipts_dense(LN), lists=one_parent(LN), scan=(65,), order=(1, LN, {0: 0, LN - 1: LN - 1}),
             claims=[("on_the_path", at(_on), 65)] + ([("off_the_path", at(_off), 1)] if _off is not None else []), plan=True, walks=1,
             drop=(lambda k: lambda where, parts: [where[("r",) + k]])(_first_child), place=_place, pos=_pos, what="first_target_missing", n=LN)
        # a hole: the first child's link and bit taken out — a well-formed sparse tree without the receipts under it
        _gone = min(_span, LN - _base)
        if _base == 0:
            case(f"link_node_{_tag}_hole_at_its_first_link", "links",
                 receipts=receipts_of((lambda g: lambda: {i: R(i) for i in range(g, LN)})(_gone), count=LN, height=4), lists=one_parent(LN),
                 scan=(1, LN, [(_gone, LN, 1)]), order=(1, LN, {0: 0, LN - 1: LN - 1}),
                 claims=[("in_the_hole", at(0), 9), ("behind_the_hole", at(_gone), 1)], plan=True, walks=1, place=_place, pos=_pos, what="hole", n=LN)
# a 43-byte link that is no CID: `d8 2a 58 27 00 | 01 71 a0 e4 02 21 | 32 bytes` — the multihash says 33 bytes where 32 follow
# (Cid::try_from fails: an Err of the node's decode).  Its first eight bytes are the standard link's; the block it would name
# is in the witness under those very 38 bytes, so a walk that takes them for a key FINDS it.
def lying_cid(c):
    assert c[:6] == bytes.fromhex("0171a0e40220") and len(c) == 38
    return c[:5] + b"\x21" + c[6:]


def _with_a_lying_link(tree, key, which, n):
    """the tree of n receipts (tree "r") or messages ("m") whose node `key` = (height, base) spells link / value `which` so"""
    def respell(b, l, v):
        items = list(l or v)
        items[which] = items[which][:10] + b"\x21" + items[which][11:]
        return raw_node(b, items if l else [], items if v else [])

    def under_the_lying_key(st, where, child):
        st.blocks[lying_cid(child)] = st.blocks.get(child, b"")

    if tree == "r":
        def make(st, where):
            root = receipts_of({i: R(i) for i in range(n)}, respell={key: respell})(st, where)
            under_the_lying_key(st, where, where[("r", key[0] - 1, key[1] + which * 8 ** key[0])])
            return root
        return make
    return one_parent(n, respell={key: respell})


for _place, (_h, _where) in LINK_NODE_AT.items():
    for _pos, _base, _on, _off in _where:
        _tag = f"{_place}_{_pos}" if _place != "root" else "root"
        case(f"link_node_{_tag}_first_link_whose_multihash_length_lies", "links", receipts=_with_a_lying_link("r", (_h, _base), 0, LN), lists=one_parent(LN),
             scan=(66,), order=(1, LN, {0: 0, LN - 1: LN - 1}),
             claims=[("on_the_path", at(_on), 66)] + ([("off_the_path", at(_off), 1)] if _off is not None else []),
             plan=_place != "root", walks=0 if _place == "root" else 1, place=_place, pos=_pos, what="multihash_length_lies", n=LN)
case("link_node_level_last_link_of_a_full_node_whose_multihash_length_lies", "links", receipts=_with_a_lying_link("r", (1, 31 * 64), 7, LN), lists=one_parent(LN),
     scan=(66,), order=(1, LN, {0: 0, LN - 1: LN - 1}), claims=[("on_the_path", at(31 * 64), 66), ("off_the_path", at(5000), 1)], plan=True, walks=1,
     place="level", pos="ending_a_workgroup_last_link", what="multihash_length_lies", n=LN)
for _pos, _base in (("first", 0), ("ending_a_workgroup", 2040), ("last_partial", 2048)):
    case(f"message_leaf_{_pos}_first_value_whose_multihash_length_lies", "links", receipts=receipts_dense(ML), lists=_with_a_lying_link("m", (0, _base), 0, ML),
         scan=(1, ML, ALL), order=(66,), claims=[("first_of_the_leaf", at(_base), 66), ("in_another_leaf", at(1000), 66)], plan=True, walks=1,
         place="message_leaf", pos=_pos, what="multihash_length_lies", n=ML)

# message-list leaves (k_dense_link_leaves: one lane per value; 2049 messages = 257 leaves, lanes 2040-2047 end workgroup 7)
ML = 2049
MSG_LEAF_SPELLINGS = {
    "bitmap_one_byte_long": (lambda b, l, v: raw_node(b + b"\x00", l, v), 66),
    "bitmap_one_byte_short": (lambda b, l, v: raw_node(b"", l, v), 66),
    "one_value_more_than_bits": (lambda b, l, v: raw_node(bytes([b[0] >> 1]), l, v), 66),
    "one_value_fewer_than_bits": (lambda b, l, v: raw_node(b, l, v[:-1]) if len(v) > 1 else raw_node(bytes([b[0] | 2]), l, v), 66),
    "first_value_with_a_two_byte_length_head": (lambda b, l, v: raw_node(b, l, [_two_byte_link(v[0])] + v[1:]), 1),
    "last_value_a_36_byte_link": (lambda b, l, v: raw_node(b, l, v[:-1] + [link(bytes.fromhex("01711220") + bytes(32))]), 1),
    "a_value_that_is_a_byte_string": (lambda b, l, v: raw_node(b, l, [bstr(v[0][4:])] + v[1:]), 66),
    "a_link_in_front_of_its_values": (lambda b, l, v: raw_node(b, [link(OTHER)], v), 66),
    "a_trailing_byte": (lambda b, l, v: raw_node(b, l, v, trailer=b"\x00"), 66),
}
for _what, (_fn, _st) in MSG_LEAF_SPELLINGS.items():
    for _pos, _base in (("first", 0), ("ending_a_workgroup", 2040), ("last_partial", 2048)):
        _len = ML
        _positions = {0: 0, ML - 1: ML - 1}
        if _what == "last_value_a_36_byte_link":  # (another CID at that place: the message there is not MSG(i))
            _positions = {0: 0} if _base == 2048 else {0: 0, ML - 1: ML - 1}
        case(f"message_leaf_{_pos}_{_what}", "links", receipts=receipts_dense(ML), lists=one_parent(ML, respell={(0, _base): _fn}),
             scan=(1, ML, ALL), order=(1, _len, _positions) if _st == 1 else (_st,),
             claims=[("first_of_the_leaf", at(_base), _st if not (_what == "last_value_a_36_byte_link" and _base == 2048) else 7), ("in_another_leaf", at(1000), _st)],
             plan=True, walks=1, place="message_leaf", pos=_pos, what=_what, n=ML)
# a 36-byte value first and in the middle of a leaf (last: above): another CID stands at that place of the execution order
def _odd_value(k):
    return lambda b, l, v: raw_node(b, l, v[:k] + [link(bytes.fromhex("01711220") + bytes([k + 1]) * 32)] + v[k + 1:])


for _pos, _base in (("first", 0), ("ending_a_workgroup", 2040)):
    for _which, _k in (("first", 0), ("middle", 4)):
        case(f"message_leaf_{_pos}_{_which}_value_a_36_byte_link", "links", receipts=receipts_dense(ML), lists=one_parent(ML, respell={(0, _base): _odd_value(_k)}),
             scan=(1, ML, ALL), order=(1, ML, {1000: 1000, ML - 1: ML - 1}),
             claims=[("the_message_that_stood_there", at(_base + _k), 7), ("beside_it", at(_base + _k + 1), 1), ("in_another_leaf", at(1000), 1)],
             plan=True, walks=1, place="message_leaf", pos=_pos, what=f"{_which}_value_a_36_byte_link", n=ML)
# a hole: one value and its bit taken out — a well-formed sparse list; the messages behind it move up one place.  (The partial
# last leaf holds one value: there the list is two longer, 2048-2050, and 2049 is the hole.)
for _pos, _n, _hole in (("first", ML, 3), ("ending_a_workgroup", ML, 2043), ("last_partial", ML + 2, 2049)):
    case(f"message_leaf_{_pos}_hole", "links", receipts=receipts_dense(ML),
         lists=parents_of([(seq(0, _n), [])], bls0=(lambda n, hole: lambda st, where: message_list(st, {i: link(MSG(i)) for i in range(n) if i != hole}, where, tag="bls0", count=n))(_n, _hole)),
         scan=(1, ML, ALL), order=(1, _n - 1, {0: 0, _hole - 1: _hole - 1, _hole: _hole + 1, _n - 2: _n - 1}),
         claims=[("in_front_of_the_hole", at(_hole - 1), 1), ("the_message_of_the_hole", at(_hole), 7),
                 ("in_another_leaf", {"e": 1000 - (1 if _hole < 1000 else 0), "msg": 1000}, 1)]  # (behind the hole: one place up)
         + ([("behind_the_hole", {"e": _hole, "msg": _hole + 1}, 1)] if _hole < ML else []),
         plan=True, walks=1, place="message_leaf", pos=_pos, what="hole", n=ML)
for _pos, _base in (("first", 0), ("ending_a_workgroup", 2040), ("last_partial", 2048)):
    case(f"message_leaf_{_pos}_missing", "links", receipts=receipts_dense(ML), lists=one_parent(ML, count=ML), scan=(1, ML, ALL), order=(65,),
         claims=[("any", at(1000), 65)], plan=True, walks=1, drop=(lambda b: lambda where, parts: [where[("m", 0, b)]])(_base),
         place="message_leaf", pos=_pos, what="missing", n=ML)

INTERIOR_SPELLINGS = frozenset(LINK_SPELLINGS) | {"first_link_of_36_bytes", "middle_link_of_36_bytes", "last_link_of_36_bytes", "first_target_missing",
                                                   "hole", "multihash_length_lies"}
MESSAGE_LEAF_SPELLINGS = frozenset(MSG_LEAF_SPELLINGS) | {"first_value_a_36_byte_link", "middle_value_a_36_byte_link", "hole", "missing", "multihash_length_lies"}

# ===== shared blocks: a tree whose equal leaves are one block =====================================================================
BIG = 65537


def _same(differ_at=None):
    return lambda: {i: (pyamt.receipt(gas=5, events_root=EV_ROOT) if i == differ_at else SAME) for i in range(BIG)}


# 65537 identical receipts: one full leaf, one full node per height 1-4, the root, the last leaf and its four ancestors
case("shared_65537_identical_receipts", "shared", receipts=receipts_of(_same()), lists=one_parent(BIG), scan=(1, BIG, ALL),
     order=(1, BIG, {0: 0, BIG - 1: BIG - 1}), claims=usual_claims(BIG), plan=True, walks=1, n=BIG, tree_blocks=11)
for _i in (0, 32768, 65536):
    case(f"shared_65537_identical_receipts_but_{_i}", "shared", receipts=receipts_of(_same(_i)), lists=one_parent(BIG), scan=(1, BIG, ALL),
         order=(1, BIG, {0: 0, BIG - 1: BIG - 1}), claims=usual_claims(BIG) + [("the_other_one", at(_i), 1)], plan=True, walks=1, n=BIG)
# a message list whose leaves repeat: 128 entries, the same 8 messages 16 times over → 8 executed messages
case("shared_message_list_of_16_equal_leaves", "shared", receipts=receipts_dense(8), lists=parents_of([(seq(0, 8) * 16, [])]), scan=(1, 8, ALL),
     order=(1, 8, {0: 0, 7: 7}), claims=[("first", at(0), 1), ("last", at(7), 1), ("raw_position_in_the_second_leaf", {"e": 8, "msg": 0}, 8)],
     plan=True, walks=1, n=8)

# ===== sparse trees: the general walk ================================================================================================
# (the walk's prefix sum is ONE workgroup up to 4096 entries and tiles of 1024 entries beyond: csrc/kernels/scan.hip)
for _stride, _tag in ((8, "leaf_node"), (64, "height_1_node")):
    for _k in (1023, 1024, 1025, 2049) + ((4095, 4096, 4097, 5119, 5120, 5121) if _stride == 8 else ()):
        _top = _stride * (_k - 1)
        case(f"sparse_one_value_per_{_tag}_{_k}_nodes", "sparse", receipts=receipts_of((lambda s, k: lambda: {s * j: R(j) for j in range(k)})(_stride, _k)),
             lists=one_parent(2 * _stride + 1), scan=(1, _top + 1, [(0, _top + 1, _stride)]), order=(1, 2 * _stride + 1, {0: 0, 2 * _stride: 2 * _stride}),
             claims=[("first", at(0), 1), ("second", at(_stride), 1), ("third", at(2 * _stride), 1), ("between", at(1), 9), ("before_the_third", at(2 * _stride - 1), 9)],
             plan=True, walks=1, stride=_stride, nodes=_k)
for _k in range(1, 8):
    for _i, _tag in ((8 ** _k, f"8_pow_{_k}"), (8 ** _k - 1, f"8_pow_{_k}_minus_1")):
        case(f"sparse_single_index_{_tag}", "sparse", receipts=receipts_of({_i: R(0)}), lists=one_parent(9), scan=(1, _i + 1, [(_i, _i + 1, 1)]),
             order=(1, 9, {0: 0, 8: 8}), claims=[("at_0", at(0), 9 if _i else 1), ("at_7", at(7), 1 if _i == 7 else 9), ("at_8", at(8), 1 if _i == 8 else 9)],
             plan=True, walks=1, index=_i)

# ===== two defects in one tree of 65537 receipts: the status depth-first `for_each` meets FIRST ====================================
# low: index 8 (the second leaf) or the height-1 node over 64-127, deep in the tree; high: the leaf of 65528-65535, or the root's
# second child (height 4, 32768-65535)
DEFECTS = {  # kind: (status, is it a leaf defect)
    "missing_leaf": (65, True), "undecodable_leaf": (66, True), "missing_interior": (65, False), "undecodable_interior": (66, False),
    "receipt_of_the_wrong_type": (66, True)}


def _defect(kind, low):
    """→ (build_amt keyword arguments, node key to drop or None, item overrides, a claimed index on its path)"""
    leaf = DEFECTS[kind][1]
    key = ((0, 8) if leaf else (1, 64)) if low else ((0, 65528) if leaf else (4, 32768))
    on = key[1] + 1
    if kind.startswith("missing"):
        return {}, key, {}, on
    if kind.startswith("undecodable"):
        return {"respell": {key: lambda b, l, v: BAD + b"node"}}, None, {}, on
    return {}, None, {key[1] + 1: RECEIPT_3}, on


def _two(name, first, second, family="two"):
    (kw1, d1, it1, on1), (kw2, d2, it2, on2) = _defect(first, True), _defect(second, False)
    kw = {"respell": {**kw1.get("respell", {}), **kw2.get("respell", {})}}
    st1, st2 = DEFECTS[first][0], DEFECTS[second][0]
    case(name, family, receipts=receipts_of((lambda over: lambda: {**{i: R(i) for i in range(BIG)}, **over})({**it1, **it2}), **kw), lists=one_parent(BIG),
         scan=(st1,), order=(1, BIG, {0: 0, BIG - 1: BIG - 1}),
         claims=[("on_the_low_defect", at(on1), st1), ("on_the_high_defect", at(on2), st2), ("on_neither", at(20000), 1)], plan=True, walks=1,
         drop=lambda where, parts: [where[("r",) + d] for d in (d1, d2) if d], low=first, high=second, n=BIG)


_kinds = list(DEFECTS)
for _a in range(len(_kinds)):
    for _b in range(_a + 1, len(_kinds)):
        _two(f"two_low_{_kinds[_a]}_high_{_kinds[_b]}", _kinds[_a], _kinds[_b])
        _two(f"two_low_{_kinds[_b]}_high_{_kinds[_a]}", _kinds[_b], _kinds[_a])
# … and across two message lists: the first list in key order decides (parents in order, BLS before secp)
def _bad_list(which, how):
    def make(st, where):
        root = message_list(st, seq({"bls0": 0, "secp0": 100, "bls1": 200}[which], 20), where, tag=which,
                            respell={(0, 8): (lambda b, l, v: BAD + b"leaf")} if how == 66 else None)
        if how == 65:
            del st.blocks[where[(which, 0, 8)]]
        return root
    return make


for _l1, _s1, _l2, _s2 in (("bls0", 65, "bls1", 66), ("bls0", 66, "bls1", 65), ("bls0", 65, "secp0", 66), ("bls0", 66, "secp0", 65), ("secp0", 65, "bls1", 66),
                           ("secp0", 66, "bls1", 65)):
    case(f"two_lists_{_l1}_{_s1}_then_{_l2}_{_s2}", "two", receipts=receipts_dense(60), lists=parents_of([(seq(0, 20), seq(100, 20)), (seq(200, 20), [])],
         **{_l1: _bad_list(_l1, _s1), _l2: _bad_list(_l2, _s2)}), scan=(1, 60, ALL), order=(_s1,), claims=[("any", at(0), _s1)], plan=True, walks=1, n=60)

# ===== receipt ranges ================================================================================================================
# A ranged scan answers as `for_each` restricted to the nodes on the paths of [lo, hi): a node on such a path is decoded whole,
# a node off those paths is never read.  has[i - lo] is receipt i (include/ipcfp.h).
def _ranged(name, n, lo, hi, **kw):
    got = max(0, min(hi, n) - lo)
    claims = [("first_of_the_range", at(lo), 1), ("last_of_the_range", at(min(hi, n) - 1), 1)] if got else []
    case(name, "ranges", receipts=receipts_dense(n), lists=one_parent(n), scan=(1, got, ALL), order=(1, n, {0: 0, n - 1: n - 1}), claims=claims,
         rng=(lo, hi), plan=got > 0, walks=1 if got else 0, n=n, **kw)


for _n in (513, 4097, 65537):
    for _B in (8, 64, 512):
        for _lo, _hi in ((_B, _B + 8), (_B - 1, _B + 8), (_B + 1, _B + 8), (_B - 8, _B), (_B - 8, _B - 1), (_B - 8, _B + 1)):
            _ranged(f"range_{_n}_from_{_lo}_to_{_hi}", _n, _lo, _hi, boundary=_B)
    _ranged(f"range_{_n}_one_receipt_before_a_64_boundary", _n, 63, 64)
    _ranged(f"range_{_n}_one_receipt_behind_a_64_boundary", _n, 64, 65)
    _ranged(f"range_{_n}_inside_one_leaf", _n, 17, 21)
    _ranged(f"range_{_n}_ending_at_count", _n, _n - 5, _n)
    _ranged(f"range_{_n}_ending_at_u64_max", _n, _n - 5, U64)
    _ranged(f"range_{_n}_wholly_behind_count", _n, _n + 3, _n + 10)
    _ranged(f"range_{_n}_whole", _n, 0, _n)
    _ranged(f"range_{_n}_across_the_middle", _n, _n // 3 + 1, 2 * _n // 3 + 2)

# defects under the range [1003, 2997) of 4097 and 65537 receipts.  On its paths: the leaves 1000-1007 … 2992-2999, the height-1
# nodes 960-1023 … 2944-3007, the height-2 nodes 512-1023 … 2560-3071, and the nodes above them.
RLO, RHI = 1003, 2997


def _malformed_link(lk):
    return b"\xd8\x2a" + bstr(lk[5:])  # no multibase byte in front of the CID


def _lying_link(lk):
    return lk[:10] + b"\x21" + lk[11:]  # (as lying_cid: the multihash says 33 bytes where 32 follow)


RANGE_DEFECTS = {  # name: (build_amt kw, item overrides, node key to drop, status of the scan, of a claim at lo, of a claim at hi - 1)
    # inside the range
    "inside_a_receipt_of_the_wrong_type": ({}, {2000: RECEIPT_3}, None, 66, 1, 1),
    "inside_a_36_byte_link": ({"odd_links": {(0, 2000)}}, {}, None, 1, 1, 1),
    "inside_a_missing_leaf": ({}, {}, (0, 2000), 65, 1, 1),
    # in an edge node, on a link or value the range does not use
    "first_leaf_a_bad_value_in_front_of_the_range": ({}, {1001: RECEIPT_3}, None, 66, 66, 1),
    "last_leaf_a_bad_value_behind_the_range": ({}, {2998: RECEIPT_3}, None, 66, 1, 66),
    "first_height_1_node_a_36_byte_link_in_front_of_the_range": ({"odd_links": {(0, 968)}}, {}, None, 1, 1, 1),
    "last_height_1_node_a_36_byte_link_behind_the_range": ({"odd_links": {(0, 3000)}}, {}, None, 1, 1, 1),
    "first_height_1_node_a_malformed_link_in_front_of_the_range":
        ({"respell": {(1, 960): lambda b, l, v: raw_node(b, [l[0], _malformed_link(l[1])] + l[2:], v)}}, {}, None, 66, 66, 1),
    "last_height_1_node_a_malformed_link_behind_the_range":
        ({"respell": {(1, 2944): lambda b, l, v: raw_node(b, l[:-1] + [_malformed_link(l[-1])], v)}}, {}, None, 66, 1, 66),
    "first_height_2_node_a_36_byte_link_in_front_of_the_range": ({"odd_links": {(1, 512)}}, {}, None, 1, 1, 1),
    "last_height_2_node_a_malformed_link_behind_the_range":
        ({"respell": {(2, 2560): lambda b, l, v: raw_node(b, l[:-1] + [_malformed_link(l[-1])], v)}}, {}, None, 66, 1, 66),
    # (a 43-byte link that is no CID keeps the node's length: nothing but a look at that very link finds it)
    "first_height_1_node_a_link_in_front_of_the_range_whose_multihash_length_lies":
        ({"respell": {(1, 960): lambda b, l, v: raw_node(b, [l[0], _lying_link(l[1])] + l[2:], v)}}, {}, None, 66, 66, 1),
    "last_height_1_node_a_link_behind_the_range_whose_multihash_length_lies":
        ({"respell": {(1, 2944): lambda b, l, v: raw_node(b, l[:-1] + [_lying_link(l[-1])], v)}}, {}, None, 66, 1, 66),
    "last_height_2_node_a_link_behind_the_range_whose_multihash_length_lies":
        ({"respell": {(2, 2560): lambda b, l, v: raw_node(b, l[:-1] + [_lying_link(l[-1])], v)}}, {}, None, 66, 1, 66),
    "first_height_1_node_an_unused_leaf_missing": ({}, {}, (0, 968), 1, 1, 1),
    "last_height_1_node_an_unused_leaf_missing": ({}, {}, (0, 3000), 1, 1, 1),
    # in a node no in-range path touches
    "off_every_path_a_receipt_of_the_wrong_type": ({}, {9: RECEIPT_3}, None, 1, 1, 1),
    "off_every_path_an_undecodable_leaf": ({"respell": {(0, 3008): lambda b, l, v: BAD + b"leaf"}}, {}, None, 1, 1, 1),
    "off_every_path_a_missing_height_1_node": ({}, {}, (1, 3072), 1, 1, 1),
}
for _n in (4097, 65537):
    for _what, (_kw, _over, _drop, _st, _c_lo, _c_hi) in RANGE_DEFECTS.items():
        case(f"range_{_n}_defect_{_what}", "ranges", receipts=receipts_of((lambda n, over: lambda: {**{i: R(i) for i in range(n)}, **over})(_n, _over), **_kw),
             lists=one_parent(_n), scan=(1, RHI - RLO, ALL) if _st == 1 else (_st,), order=(1, _n, {0: 0, _n - 1: _n - 1}),
             claims=[("first_of_the_range", at(RLO), _c_lo), ("last_of_the_range", at(RHI - 1), _c_hi)],
             rng=(RLO, RHI), plan=True, walks=1, drop=(lambda d: (lambda where, parts: [where[("r",) + d]]) if d else None)(_drop), n=_n, defect=_what)


# … and in 513 receipts under [67, 117): the leaves 64-71 … 112-119, the height-1 node 64-127 and the root
for _what, _kw, _over, _st, _c_lo, _c_hi in (
        ("first_leaf_a_bad_value_in_front_of_the_range", {}, {65: RECEIPT_3}, 66, 66, 1),
        ("last_leaf_a_bad_value_behind_the_range", {}, {118: RECEIPT_3}, 66, 1, 66),
        ("last_height_1_node_a_link_behind_the_range_whose_multihash_length_lies",
         {"respell": {(1, 64): lambda b, l, v: raw_node(b, l[:-1] + [_lying_link(l[-1])], v)}}, {}, 66, 66, 66),
        ("first_height_2_node_a_36_byte_link_in_front_of_the_range", {"odd_links": {(1, 0)}}, {}, 1, 1, 1),
        ("off_every_path_a_receipt_of_the_wrong_type", {}, {9: RECEIPT_3}, 1, 1, 1)):
    case(f"range_513_defect_{_what}", "ranges", receipts=receipts_of((lambda over: lambda: {**{i: R(i) for i in range(513)}, **over})(_over), **_kw),
         lists=one_parent(513), scan=(1, 50, ALL) if _st == 1 else (_st,), order=(1, 513, {0: 0, 512: 512}),
         claims=[("first_of_the_range", at(67), _c_lo), ("last_of_the_range", at(116), _c_hi)], rng=(67, 117), plan=True, walks=1, n=513, defect=_what)


def _off_path_nodes(lo, hi):
    """every node of the receipts tree whose span does not meet [lo, hi)"""
    def drop(where, parts):
        meets = lambda key: key[2] < hi and key[2] + 8 ** (key[1] + 1) > lo  # noqa: E731
        on = {cid for key, cid in where.items() if key[0] == "r" and meets(key)}
        return {cid for key, cid in where.items() if key[0] == "r" and not meets(key)} - on
    return drop


# a shard's witness: every block off the range's paths deleted
for _n in (4097, 65537):
    case(f"range_{_n}_on_a_witness_without_the_off_path_blocks", "ranges", receipts=receipts_dense(_n), lists=one_parent(_n), scan=(1, RHI - RLO, ALL),
         order=(1, _n, {0: 0, _n - 1: _n - 1}), claims=[("first_of_the_range", at(RLO), 1), ("last_of_the_range", at(RHI - 1), 1)], rng=(RLO, RHI),
         plan=True, walks=1, drop=_off_path_nodes(RLO, RHI), n=_n, shard_witness=True)

FAMILIES = collections.Counter(c.family for c in CASES.values())
