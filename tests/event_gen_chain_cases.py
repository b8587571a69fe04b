"""Chains of tipset PAIRS for the event generator over a chain (ipcfp_generate_event_claims_tipsets), buildable on the CPU.

Every pair of every chain lives in ONE merged store (as scan_tipsets_cases.world() makes one): a chain is a list of pair
names, and the expected answer of tipset t is pyevents.generate(merged blocks, parents_t, child_t, filter).  The pairs come
from event_chain_cases.tipset(salt=…); every pair has messages, receipts and headers of its own (unique message tags and
emitters), so that a block dropped from one pair is in no other pair either.  The shared-message pairs (`shared/…`) carry
ONE message CID in two different tipsets and duplicate it inside each (DUP_BLS / DUP_SECP / DUP_PARENTS re-tagged once).

The failing kinds, each the single call's status:
    child_absent, child_undecodable, parent_absent, txmeta_absent, msg_node_undecodable, receipts_absent,
    events/k (scan_multi_cases.err_tipsets: the events phase of the scan), beyond (a match at a receipt index beyond the
    execution order: "Missing message at index").
"A base CID absent from the witness" is NOT among them because no input reaches it: the base CIDs are the parents, the child
and the receipts root, and a tipset that arrives at the marks has loaded every one of them in an earlier step (pyevents.generate
shows the same: its materialise loop cannot raise).  The per-tipset missing flag keeps the single call's rule in the code.

`expected_chain` lays the per-tipset answers end to end: the contract of include/ipcfp.h."""
import functools

import event_chain_cases as ec
import pyamt
import pyevents
import scan_multi_cases as mc

MAX_TIPSETS = 4096
FILTER = ec.FILTER
NO_MATCH_TOPICS = (2, 3)  # what a pair without a match carries in topics 0 and 1


def _msgs(uid, shape):
    """shape: per parent (n_bls, n_secp) → unique message CIDs"""
    out, k = [], 0
    for nb, ns in shape:
        bls = [ec.M(f"gen{uid}/{k + i}") for i in range(nb)]
        k += nb
        secp = [ec.M(f"gen{uid}/{k + i}") for i in range(ns)]
        k += ns
        out.append((bls, secp))
    return out


def _receipts(uid, indices, match=True, n_events=1):
    topics = (0, 1) if match else NO_MATCH_TOPICS
    def one(i):
        return lambda st: pyamt.receipt(gas=uid, events_root=ec.events_root(st, {j: ec.good_event(100000 + 1000 * uid + i + j, topics=topics, n_data=8)
                                                                                  for j in range(n_events)}))
    return {i: one(i) for i in indices}


_PAIRS = []  # (name, callable(uid) → (store, parts))


def _pair(name, **kw):
    shape = kw.pop("shape", ((3, 1), (2, 1)))
    receipts_at = kw.pop("receipts_at", None)
    match = kw.pop("match", True)
    n_events = kw.pop("n_events", 1)
    msgs = kw.pop("msgs", None)

    def make(uid):
        m = msgs(uid) if msgs else _msgs(uid, shape)
        n_exec = len(ec.first_seen(m))
        at = receipts_at(n_exec) if receipts_at else range(n_exec)
        extra = {k: (v(uid) if k in ("msg_amt",) else v) for k, v in kw.items()}
        st, _claim, parts = ec.tipset(msgs=m, receipts=_receipts(uid, at, match, n_events), salt=1000 + 7 * uid, at=(0, 0),
                                      event=ec.SIB, **extra)
        return st, parts
    _PAIRS.append((name, make))


def _retag(template, tag):
    """a DUP_* message layout with its message CIDs re-tagged, the SAME for every uid (so two pairs share every message CID)"""
    names = {}
    def m(c):
        return names.setdefault(c, ec.M(f"{tag}/{len(names)}"))
    return lambda uid: [([m(c) for c in bls], [m(c) for c in secp]) for bls, secp in template]


# sound pairs: 17 distinct ones for the sound chains
for _k in range(17):
    _pair(f"ok/{_k}", shape=(((3, 1), (2, 1)), ((1, 0),), ((2, 2), (0, 1), (1, 1)))[_k % 3])
# one message CID in two different tipsets, duplicated inside each, across BLS / secp and across parents
_pair("shared/bls_a", msgs=_retag(ec.DUP_BLS, "shared_bls"))
_pair("shared/bls_b", msgs=_retag(ec.DUP_BLS, "shared_bls"))
_pair("shared/secp_a", msgs=_retag(ec.DUP_SECP, "shared_secp"))
_pair("shared/secp_b", msgs=_retag(ec.DUP_SECP, "shared_secp"))
_pair("shared/parents_a", msgs=_retag(ec.DUP_PARENTS, "shared_parents"))
_pair("shared/parents_b", msgs=_retag(ec.DUP_PARENTS, "shared_parents"))
_pair("nine", msgs=_retag(ec.NINE_MSGS, "nine"))
# empty message trees (no receipts either: nothing executed) and pairs without a match
for _k in range(3):
    _pair(f"empty/{_k}", shape=((0, 0),))
    _pair(f"nomatch/{_k}", match=False)
# parent counts (33: the wide form)
for _p in (1, 2, 5, 32, 33):
    _pair(f"parents/{_p}", shape=((1, 0),) * _p)
# raw message positions: tipsets of 31, 1, 1 and of 1023, 1, 1, 1024, 1025 messages (receipts at the first and last index only)
_ENDS = lambda n: sorted({0, n - 1})  # noqa: E731
for _n in (31, 1023, 1024, 1025):
    _pair(f"msgs/{_n}", shape=((_n, 0),), receipts_at=_ENDS)
for _k in range(5):
    _pair(f"msgs/1/{_k}", shape=((1, 0),))
# match counts: one receipt with many matching events
for _n in (600, 424, 500, 3):
    _pair(f"events/{_n}", shape=((1, 0),), n_events=_n)
# 8 tiny pairs for the chain of MAX_TIPSETS
for _k in range(8):
    _pair(f"tiny/{_k}", shape=((1 + _k % 2, _k % 3 == 0),))
# failing pairs
_pair("fail/child_absent", drop=("child",))
_pair("fail/child_undecodable", child_header=lambda f: ec.BAD)
_pair("fail/parent_absent", drop=("parent1",))
_pair("fail/txmeta_absent", drop=("txmeta0",))
_pair("fail/msg_node_undecodable",
      msg_amt=lambda uid: (lambda st, k, which, cids: st.put(ec.BAD + b"node %d" % uid) if (k, which) == (1, "bls") else None))
_pair("fail/receipts_absent", drop=("receipts",))
_pair("fail/beyond", receipts_at=lambda n: range(n + 2))  # two receipts more than messages, each with a match

FAIL_KINDS = ("fail/child_absent", "fail/child_undecodable", "fail/parent_absent", "fail/txmeta_absent", "fail/msg_node_undecodable",
              "fail/receipts_absent", "fail/events/0", "fail/beyond")
ERR, ERR_MISSING_BLOCK, ERR_DECODE = 64, 65, 66  # ipcfp_status_t (include/ipcfp.h)
WANT_STATUS = {"fail/child_absent": ERR_MISSING_BLOCK, "fail/child_undecodable": ERR_DECODE, "fail/parent_absent": ERR_MISSING_BLOCK,
               "fail/txmeta_absent": ERR_MISSING_BLOCK, "fail/msg_node_undecodable": ERR_DECODE, "fail/receipts_absent": ERR_MISSING_BLOCK,
               "fail/beyond": ERR}


@functools.lru_cache(maxsize=None)
def world():
    """→ (merged store, {pair name: ([parent CIDs], child CID)})"""
    store, pairs, dropped = pyamt.Store(), {}, set()

    def take(blocks):
        for cid, block in blocks.items():
            assert store.blocks.setdefault(cid, block) == block

    for uid, (name, make) in enumerate(_PAIRS):
        st, parts = make(uid)
        take(st.blocks)
        dropped |= set(parts["dropped"])
        pairs[name] = (list(parts["parents"]), parts["child"])
    for k, (_name, st, parts) in enumerate(mc.err_tipsets()):
        take(st.blocks)
        dropped |= set(parts["dropped"])
        pairs[f"fail/events/{k}"] = (list(parts["parents"]), parts["child"])
    assert not (dropped & set(store.blocks)), "a dropped block came back with another pair"
    assert len({(tuple(p), c) for p, c in pairs.values()}) == len(pairs)
    return store, pairs


@functools.lru_cache(maxsize=None)
def raw_positions(name):
    """raw message positions of a pair: Σ over parents of its BLS and secp list lengths, read off the merged store"""
    store, pairs = world()
    total = 0
    for p in pairs[name][0]:
        tx = pyevents.header(store.blocks[p]).messages
        for root in pyevents.txmeta_roots(store.blocks[tx]):
            total += sum(1 for _ in pyevents.amt_for_each(pyevents.amt_load(store.blocks, root, 0, pyevents.check_cid_value)))
    return total


# ---- chains -------------------------------------------------------------------------------------------------------------------------
OK = [f"ok/{k}" for k in range(17)]
TINY = [f"tiny/{k}" for k in range(8)]


def cycle(pool, n, start=0):
    return [pool[(start + i) % len(pool)] for i in range(n)]


def _places(special, n_special=1):
    """a special pair (or pairs) in first / middle / last place between sound ones"""
    sp = special if isinstance(special, list) else [special]
    return {"first": sp[:1] + OK[:2], "middle": OK[:1] + sp[:1] + OK[1:2], "last": OK[:2] + sp[:1]}


def _chains():
    out = {}

    def chain(name, tipsets):
        assert name not in out
        out[name] = list(tipsets)

    _store, pairs = world()
    for p in pairs:  # T = 1 for every pair: must equal the single call
        chain(f"one/{p}", [p])
    chain("sound/2", OK[:2])
    chain("sound/3", OK[2:5])
    chain("sound/17", OK)
    chain("same_pair/adjacent", [OK[0], OK[0], OK[1]])
    chain("same_pair/apart", [OK[0], OK[1], "nine", OK[0]])
    chain("shared_message/bls", ["shared/bls_a", OK[0], "shared/bls_b"])
    chain("shared_message/secp", ["shared/secp_a", "shared/secp_b"])
    chain("shared_message/parents", ["shared/parents_a", "nine", "shared/parents_b", "shared/parents_a"])
    for place, c in _places("empty/0").items():
        chain(f"empty/{place}", c)
    chain("empty/all", ["empty/0", "empty/1", "empty/2"])
    for place, c in _places("nomatch/0").items():
        chain(f"nomatch/{place}", c)
    chain("nomatch/all", ["nomatch/0", "nomatch/1", "nomatch/2"])
    for kind in FAIL_KINDS:
        for place, c in _places(kind).items():
            chain(f"{kind}/{place}", c)
    chain("fail/two_kinds", [OK[0], "fail/txmeta_absent", OK[1], "fail/beyond", OK[2], "fail/events/1"])
    chain("fail/every_tipset", list(FAIL_KINDS))
    chain("edges/31+1+1", ["msgs/31", "msgs/1/0", "msgs/1/1", OK[0]])
    chain("edges/1023+1+1+1024+1025", ["msgs/1023", "msgs/1/0", "msgs/1/1", "msgs/1024", "msgs/1025"])
    chain("matches/1024_at_a_boundary", ["events/600", "events/424", "events/3", OK[0]])
    chain("matches/1024_inside_a_tipset", ["events/600", "events/500", "events/3"])
    chain("parent_counts", [f"parents/{p}" for p in (1, 2, 5, 32, 33)])
    chain(f"tiny/{MAX_TIPSETS}", cycle(TINY, MAX_TIPSETS))
    return out


@functools.lru_cache(maxsize=None)
def chains():
    """→ {name: [pair name]}"""
    return _chains()


SINGLE_CALL_LIMIT = 64  # chains up to this length are also held to T single calls on the GPU


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_pair(name, actor=None):
    """→ (status, rows [(exec_index, event_index, emitter, message CID)], needed CIDs) of one pair over the MERGED blocks"""
    store, pairs = world()
    parents, child = pairs[name]
    st, proofs, needed = pyevents.generate(store.blocks, parents, child, *FILTER, actor)
    if st != pyevents.TRUE:
        return st, (), frozenset()
    return st, tuple(proofs), frozenset(needed)


def cid_ord_key(cid: bytes):
    """`Cid: Ord` (version, codec, multihash code, size, digest) of a binary CIDv1 with one-byte varints or a CIDv0"""
    if cid[:2] == b"\x12\x20":
        return (0, 0x70, 0x12, 32, cid[2:])
    pos, vals = 0, []
    for _ in range(4):
        v = shift = 0
        while True:
            b = cid[pos]
            pos += 1
            v |= (b & 0x7f) << shift
            shift += 7
            if not b & 0x80:
                break
        vals.append(v)
    return (*vals, cid[pos:pos + vals[3]])


def expected_chain(name, actor=None):
    """the per-tipset answers laid end to end → dict(status, claim_off, rows, per_tipset rows, needed: CIDs in `Cid: Ord` order)"""
    out = {"status": [], "claim_off": [0], "rows": [], "per_tipset": [], "needed": set()}
    for p in chains()[name]:
        st, rows, needed = expected_pair(p, actor)
        out["status"].append(st)
        out["per_tipset"].append(list(rows))
        out["rows"] += list(rows)
        out["claim_off"].append(len(out["rows"]))
        out["needed"] |= needed
    out["needed"] = sorted(out["needed"], key=cid_ord_key)
    return out


def layout(status, n_match, blob_bytes):
    """csrc/host/gen_tipsets_layout.h restated → (claim_off, blob_off, n_sound, first_failing)"""
    c_off, b_off, sound_n, first = [0], [0], 0, -1
    for t, (st, m, b) in enumerate(zip(status, n_match, blob_bytes)):
        sound = st == pyevents.TRUE
        if not sound and first < 0:
            first = t
        sound_n += sound
        c_off.append(c_off[-1] + (m if sound else 0))
        b_off.append(b_off[-1] + (b if sound else 0))
    return c_off, b_off, sound_n, first


# literal expectations of the small chains (read off event_chain_cases: execution orders and emitters are written out here)
def _emitter(pair, i):
    return 100000 + 1000 * [n for n, _ in _PAIRS].index(pair) + i


LITERAL = {
    # ok/0: two parents ([m0 m1 m2], [m3]) ([m4 m5], [m6]): 7 messages, 7 receipts, one match each
    "sound/2": {"status": [1, 1], "claim_off": [0, 7, 8],
                "triples": [(i, 0, _emitter("ok/0", i)) for i in range(7)] + [(0, 0, _emitter("ok/1", 0))]},
    "empty/all": {"status": [1, 1, 1], "claim_off": [0, 0, 0, 0], "triples": []},
    "nomatch/all": {"status": [1, 1, 1], "claim_off": [0, 0, 0, 0], "triples": []},
    "fail/beyond/middle": {"status": [1, pyevents.ERR, 1], "claim_off": [0, 7, 7, 8],
                           "triples": [(i, 0, _emitter("ok/0", i)) for i in range(7)] + [(0, 0, _emitter("ok/1", 0))]},
    # DUP_BLS = [([A B A C], [D])]: execution order A B C D in both tipsets, although they share every message CID
    "shared_message/bls": {"status": [1, 1, 1], "claim_off": [0, 4, 11, 15],
                           "triples": [(i, 0, _emitter("shared/bls_a", i)) for i in range(4)] + [(i, 0, _emitter("ok/0", i)) for i in range(7)] +
                                      [(i, 0, _emitter("shared/bls_b", i)) for i in range(4)]},
}
