"""A plain, slow restatement of the event side of the reference in Python: the second judge of the event chain next to the
C++ oracle.  Written from the reference's Rust —

    verify_event_proof            src/proofs/events/verifier.rs:92-290
    reconstruct_execution_order   src/proofs/events/utils.rs:16-94  (collect_exec_list, verify_txmeta = true)
    find_matching_events          src/proofs/events/generator.rs:180-307, matches_log :38-40
    extract_evm_log               src/proofs/common/evm.rs:13-59
    HeaderLite                    src/proofs/common/decode.rs:100-118

and SURVEY.md A.5, A.8-A.10.

    verify(blocks, claim, trust=None, filt=None) -> status byte (include/ipcfp.h)
    exec_order(blocks, parent cids)              -> [message cid]            (raises Err)
    scan(blocks, receipts_root, t0, t1, actor)   -> (status, has-match list, [(exec_index, event_index, emitter)], {recorded cids})
    generate(blocks, parents, child, t0, t1, a)  -> (status, [(exec_index, event_index, emitter, message cid)], {witness cids})

`claim` holds the fields of `EventProof` as the reference's struct does (strings stay strings): parent_epoch, child_epoch,
parent_tipset_cids, child_block_cid, message_cid, exec_index, event_index, emitter, topics, data.  `trust` is None
(AcceptAll) or (ec_chain_empty, min_epoch, max_epoch) (cert.rs:52-64), `filt` None or (topic0, topic1)
(create_event_filter, verifier.rs:28-39).

Like tests/pystorage.py it works on TREES: a block is decoded whole by pystorage's strict DAG-CBOR reader and the typed
decodes are shape checks on the tree.  The AMT READ side is new here (tests/pyamt.py stays the writer, nothing of its node
layout is imported): `amt_load`, `amt_get`, `amt_for_each`, with the value type checked for every value of a node when
the node is decoded, as serde does for `CollapsedNode<V>`.

HOW FAR IT IS INDEPENDENT.  The order of the verifier's steps, which string is parsed when, what is compared with what,
the first-seen dedupe, last-wins of a repeated entry key — all of that is the reference's own text and is read here from
the Rust alone.  What fvm_ipld_amt / fvm_shared / serde do INSIDE is not in that text and the crates are not at hand:
there this file follows SURVEY.md A.5/A.8 and makes the SAME choice the oracle and the engine were written to make.
Those choices have NAMES (the constants below) and a case each in tests/assumption_cases.py EVENT_CASES."""
import functools

import pyamt
import pystorage
from pystorage import ERR_BAD_CLAIM, ERR_MISSING_BLOCK, Err, _bad, _bytes, _cid, _i64, _tuple, _u64, cid_from_string

# one block is decoded many times over a batch; the trees are only ever read here (a failed decode is not kept: it raises again)
decode = functools.lru_cache(maxsize=1 << 14)(pystorage.decode)

TRUE = 1
(FALSE_UNTRUSTED_PARENT, FALSE_UNTRUSTED_CHILD, FALSE_PARENTS_MISMATCH, FALSE_CHILD_EPOCH, FALSE_PARENT_EPOCH, FALSE_MSG_NOT_IN_EXEC,
 FALSE_EXEC_INDEX, FALSE_NO_RECEIPT, FALSE_NO_EVENTS_ROOT, FALSE_NO_EVENT, FALSE_EMITTER, FALSE_NOT_EVM_LOG, FALSE_TOPIC_COUNT,
 FALSE_TOPIC, FALSE_DATA, FALSE_FILTER) = range(2, 18)
ERR, ERR_TXMETA_MISMATCH, ERR_EMPTY_PARENTS = 64, 67, 71
STATUSES = frozenset(range(1, 18)) | {64, 65, 66, 67, 69, 71}  # what verify_event_proof can answer

# ---- the named assumptions about fvm_ipld_amt / fvm_shared (tests/assumption_cases.py EVENT_CASES, one case or more each) ----
# `Amt::load` decodes the root block and compares `height` with MAX_HEIGHT; it does not look at `count`, and no get or
# for_each does either
AMT_COUNT_IS_NOT_CHECKED = True
# MAX_HEIGHT is 64 / bit_width: a root that says more is an Err of the load
AMT_MAX_HEIGHT_IS_64_OVER_BIT_WIDTH = True
# MAX_INDEX is u64::MAX - 1: `get(u64::MAX)` is Err(OutOfRange) — the generic Err, status 64 — before the tree is looked at
AMT_MAX_INDEX_IS_U64_MAX_MINUS_1 = True
# a node with links is an interior node whatever the root's height says; reaching one at height 0 is an Err of the walk
# (a get whose index the root's height cannot hold has answered None before, without looking at the node)
AMT_LINKS_AT_HEIGHT_0_ARE_AN_ERR_OF_THE_WALK = True
# a v3 root's bit width must be 1..8 (include/ipcfp.h names the upper bound an engine limit)
AMT_BIT_WIDTH_IS_1_TO_8 = True
# `Entry.flags` and `Entry.codec` are any u64 (bitflags' serde keeps unknown bits), `Receipt.exit_code` a u32
ENTRY_FLAGS_AND_CODEC_ARE_ANY_U64 = True


# ---- typed decodes ------------------------------------------------------------------------------------
class Header:
    __slots__ = ("parents", "height", "parent_state_root", "receipts", "messages", "timestamp", "fork_signaling")


def header(block: bytes) -> Header:
    """HeaderLite (common/decode.rs:100-118): a 16-tuple; five typed fields besides `parents`, eleven IgnoredAny"""
    t = _tuple(decode(block), 16, "header")
    h = Header()
    if type(t[5]) is not list:
        _bad("parents is not an array")
    h.parents = [_cid(p, "parent") for p in t[5]]
    h.height = _i64(t[7], "height")
    h.parent_state_root = _cid(t[8], "parent_state_root")
    h.receipts = _cid(t[9], "parent_message_receipts")
    h.messages = _cid(t[10], "messages")
    h.timestamp = _u64(t[12], "timestamp")
    h.fork_signaling = _u64(t[14], "fork_signaling")
    return h


def check_cid_value(x):
    return _cid(x, "AMT value")


def check_receipt(x):
    """fvm_shared `Receipt` [exit_code u32, return_data bytes, gas_used u64, events_root cid | null] → events_root or None"""
    r = _tuple(x, 4, "Receipt")
    if _u64(r[0], "exit_code") >= 1 << 32:
        _bad("exit_code does not fit u32")
    _bytes(r[1], "return_data")
    _u64(r[2], "gas_used")
    return None if r[3] is None else _cid(r[3], "events_root")


def check_stamped_event(x):
    """`StampedEvent` [emitter u64, ActorEvent]; ActorEvent is transparent `[Entry…]`, `Entry` [flags, key text, codec, value
    bytes] → (emitter, [(key, value)])"""
    s = _tuple(x, 2, "StampedEvent")
    emitter = _u64(s[0], "emitter")
    if type(s[1]) is not list:
        _bad("ActorEvent is not an array")
    entries = []
    for e in s[1]:
        e = _tuple(e, 4, "Entry")
        _u64(e[0], "flags")  # ENTRY_FLAGS_AND_CODEC_ARE_ANY_U64
        if type(e[1]) is not str:
            _bad("Entry.key is not text")
        _u64(e[2], "codec")
        entries.append((e[1], _bytes(e[3], "Entry.value")))
    return emitter, entries


def extract_evm_log(entries):
    """evm.rs:13-59 over decoded entries [(key, value)] → (topics, data) or None.  (tests/claims.py::extract_evm_log reads
    the same text from a StampedEvent's bytes; tests/event_chain_cases.py lowers its claims with that one, so the two
    restatements are held to the same literals from both ends.)"""
    m = {}
    for k, v in entries:
        m[k] = v                                              # :14-17 HashMap::insert: a repeated key keeps the LAST value
    if "topics" in m:                                         # Case A :20-30
        t = m["topics"]
        if len(t) % 32:
            return None
        return [t[i:i + 32] for i in range(0, len(t), 32)], m.get("data", b"")
    topics = []
    for key in ("t1", "t2", "t3", "t4"):                      # Case B :33-58
        if key not in m:
            break
        if len(m[key]) != 32:
            return None
        topics.append(m[key])
    if not topics:
        return None
    return topics, m.get("d", b"")


# ---- the AMT, read side ---------------------------------------------------------------------------------
class _Node:
    __slots__ = ("bits", "links", "values")


def _amt_node(x, bit_width, check_value) -> _Node:
    """`CollapsedNode<V>` `(bmap bytes, [link…], [V…])` and its `expand(bit_width)`: every value typed as V, the bitmap
    exactly ceil(2^bw / 8) bytes, links XOR values, one entry per set bit (bits past 2^bw in the last byte do not count)"""
    t = _tuple(x, 3, "AMT node")
    bmap = _bytes(t[0], "bitmap")
    if type(t[1]) is not list or type(t[2]) is not list:
        _bad("AMT node: links / values")
    nd = _Node()
    nd.links = [_cid(c, "AMT link") for c in t[1]]
    nd.values = [check_value(v) for v in t[2]]
    width = 1 << bit_width
    if nd.links and nd.values:
        _bad("AMT node has both links and values")
    if len(bmap) != (width + 7) // 8:
        _bad("AMT bitmap length")
    nd.bits = [i for i in range(width) if bmap[i >> 3] >> (i & 7) & 1]  # LSB first
    if len(nd.bits) != (len(nd.links) if nd.links else len(nd.values)):
        _bad("AMT node entry count does not match its bitmap")
    return nd


class Amt:
    __slots__ = ("bit_width", "height", "count", "node", "blocks", "check", "seen")


def amt_load(blocks, cid, version, check_value, seen=None) -> Amt:
    """`Amtv0::load` (version 0: `[height, count, node]`, bit width 3) / `Amt::load` (3: `[bit_width, height, count, node]`):
    reads the root block and nothing else.  `seen`: a set that records every CID fetched (RecordingBlockStore)."""
    if seen is not None:
        seen.add(cid)
    if cid not in blocks:
        raise Err(ERR_MISSING_BLOCK, "AMT root")
    t = decode(blocks[cid])
    a = Amt()
    if version == 0:
        t = _tuple(t, 3, "Amtv0 root")
        a.bit_width = 3
    else:
        t = _tuple(t, 4, "Amt root")
        a.bit_width = _u64(t[0], "bit_width")
        if not 1 <= a.bit_width <= 8:
            _bad("bit width")  # AMT_BIT_WIDTH_IS_1_TO_8
        t = t[1:]
    a.height = _u64(t[0], "height")
    a.count = _u64(t[1], "count")  # AMT_COUNT_IS_NOT_CHECKED
    a.node = _amt_node(t[2], a.bit_width, check_value)
    if a.height > 64 // a.bit_width:
        _bad("height above MAX_HEIGHT")  # AMT_MAX_HEIGHT_IS_64_OVER_BIT_WIDTH
    a.blocks, a.check, a.seen = blocks, check_value, seen
    return a


def _amt_child(a: Amt, cid) -> _Node:
    if a.seen is not None:
        a.seen.add(cid)
    if cid not in a.blocks:
        raise Err(ERR_MISSING_BLOCK, "AMT node")
    return _amt_node(decode(a.blocks[cid]), a.bit_width, a.check)


ABSENT = object()  # `Ok(None)` of a get (a receipt's checked value may itself be None: events_root null)


def amt_get(a: Amt, i: int):
    """→ the checked value, or ABSENT"""
    if i > (1 << 64) - 2:
        raise Err(ERR, "index out of range")  # AMT_MAX_INDEX_IS_U64_MAX_MINUS_1
    if i >= 1 << min(a.bit_width * (a.height + 1), 64):
        return ABSENT
    nd, h = a.node, a.height
    while True:
        if not nd.links:  # a leaf
            if i >= 1 << a.bit_width or i not in nd.bits:
                return ABSENT
            return nd.values[nd.bits.index(i)]
        if h == 0:
            _bad("links at height 0")  # AMT_LINKS_AT_HEIGHT_0_ARE_AN_ERR_OF_THE_WALK
        span = 1 << min(a.bit_width * h, 64)
        sub = i // span
        if sub >= 1 << a.bit_width or sub not in nd.bits:
            return ABSENT
        nd, h, i = _amt_child(a, nd.links[nd.bits.index(sub)]), h - 1, i % span


def amt_for_each(a: Amt, lo=0, hi=None):
    """yields (index, checked value) in ascending index order, depth first — the first failure in that order is the Err.
    With a range [lo, hi): a subtree whose indices lie wholly outside it is not entered (its block is not fetched), and of
    the values of a leaf that is entered those inside the range are yielded; nothing else changes — a node that IS entered is
    decoded whole."""
    def meets(base, span):
        return hi is None or (base < hi and base + span > lo)

    def walk(nd, h, base):
        if not nd.links:
            for k, i in enumerate(nd.bits):
                if meets(base + i, 1):
                    yield base + i, nd.values[k]
            return
        if h == 0:
            _bad("links at height 0")
        span = 1 << min(a.bit_width * h, 64)
        for k, i in enumerate(nd.bits):
            if meets(base + i * span, span):
                yield from walk(_amt_child(a, nd.links[k]), h - 1, base + i * span)
    yield from walk(a.node, a.height, 0)


# ---- reconstruct_execution_order (events/utils.rs:16-94) ---------------------------------------------------------------
def _get(blocks, cid, what, seen=None):
    if seen is not None:
        seen.add(cid)
    if cid not in blocks:
        raise Err(ERR_MISSING_BLOCK, what)
    return blocks[cid]


def txmeta_roots(block, cid=None):
    """`(Cid, Cid)` from the block (:61) and, with `cid`, `put_cbor(&(bls, secp), Blake2b256)` compared with it (:64-72)"""
    t = _tuple(decode(block), 2, "TxMeta")
    bls, secp = _cid(t[0], "bls root"), _cid(t[1], "secp root")
    if cid is not None and pyamt.cid_of(pyamt.array([pyamt.link(bls), pyamt.link(secp)])) != cid:
        raise Err(ERR_TXMETA_MISMATCH, "TxMeta mismatch")
    return bls, secp


def exec_order(blocks, parent_cids, verify_txmeta=True):
    txmeta = [header(_get(blocks, p, "parent header")).messages for p in parent_cids]  # :20-27: every header first
    out, seen = [], set()
    for tx in txmeta:                                                                   # :56
        bls, secp = txmeta_roots(_get(blocks, tx, "TxMeta"), tx if verify_txmeta else None)
        for root in (bls, secp):                                                        # :76-90
            for _i, c in amt_for_each(amt_load(blocks, root, 0, check_cid_value)):
                if c not in seen:                                                       # HashSet<Cid>: ONE set for all parents
                    seen.add(c)
                    out.append(c)
    return out


# ---- verify_event_proof ---------------------------------------------------------------------------------------------------
def _parse_cid(s):
    try:
        return cid_from_string(s)
    except ValueError:
        raise Err(ERR_BAD_CLAIM, "unparsable CID string")


def _trusted(trust, epoch):
    if trust is None:
        return True
    empty, lo, hi = trust
    return not empty and lo <= epoch <= hi


def _ascii_lower(s):
    return "".join(chr(ord(ch) + 32) if "A" <= ch <= "Z" else ch for ch in s)


def _verify(blocks, c, trust, filt):
    # Step 1: verify_trust_anchors (:124-144)
    parents = [_parse_cid(s) for s in c["parent_tipset_cids"]]                       # :130
    child = _parse_cid(c["child_block_cid"])                                         # :131
    if not _trusted(trust, c["parent_epoch"]):
        return FALSE_UNTRUSTED_PARENT                                                # :134
    if not _trusted(trust, c["child_epoch"]):
        return FALSE_UNTRUSTED_CHILD                                                 # :139
    # Step 2: verify_header_consistency (:147-181)
    child_hdr = header(_get(blocks, child, "child header"))                          # :155-158
    if child_hdr.parents != parents:
        return FALSE_PARENTS_MISMATCH                                                # :161
    if child_hdr.height != c["child_epoch"]:
        return FALSE_CHILD_EPOCH                                                     # :166
    if not parents:
        raise Err(ERR_EMPTY_PARENTS, "parent_cids[0] panics")                        # :172
    if header(_get(blocks, parents[0], "parent header")).height != c["parent_epoch"]:
        return FALSE_PARENT_EPOCH                                                    # :176
    # Step 3: verify_execution_order (:184-204)
    order = exec_order(blocks, parents)                                              # :190
    msg = _parse_cid(c["message_cid"])                                               # :193 — AFTER the execution order
    if msg not in order:
        return FALSE_MSG_NOT_IN_EXEC                                                 # :194
    if order.index(msg) != c["exec_index"]:
        return FALSE_EXEC_INDEX                                                      # :199
    # Step 4: verify_receipt_and_event (:207-254)
    child_hdr = header(_get(blocks, child, "child header"))                          # :214-217
    events_root = amt_get(amt_load(blocks, child_hdr.receipts, 0, check_receipt), c["exec_index"])  # :220-224
    if events_root is ABSENT:
        return FALSE_NO_RECEIPT
    if events_root is None:
        return FALSE_NO_EVENTS_ROOT                                                  # :229
    ev = amt_get(amt_load(blocks, events_root, 3, check_stamped_event), c["event_index"])  # :234-237
    if ev is ABSENT:
        return FALSE_NO_EVENT
    emitter, entries = ev
    # verify_event_data_matches (:257-290)
    if emitter != c["emitter"]:
        return FALSE_EMITTER                                                         # :262
    log = extract_evm_log(entries)
    if log is None:
        return FALSE_NOT_EVM_LOG                                                     # :267
    topics, data = log
    if len(topics) != len(c["topics"]):
        return FALSE_TOPIC_COUNT                                                     # :272
    for actual, stored in zip(topics, c["topics"]):
        if _ascii_lower("0x" + actual.hex()) != _ascii_lower(stored):
            return FALSE_TOPIC                                                       # :276-281
    if _ascii_lower("0x" + data.hex()) != _ascii_lower(c["data"]):
        return FALSE_DATA                                                            # :284-287
    if filt is not None and not matches_log(topics, filt):
        return FALSE_FILTER                                                          # :247-251
    return TRUE


def matches_log(topics, filt):
    """EventMatcher::matches_log (generator.rs:38-40) == create_event_filter's closure (verifier.rs:32-38)"""
    return len(topics) >= 2 and topics[0] == filt[0] and topics[1] == filt[1]


def verify(blocks, claim, trust=None, filt=None) -> int:
    try:
        return _verify(blocks, claim, trust, filt)
    except Err as e:
        return e.status


def claimed_event(blocks, c):
    """the checked StampedEvent (emitter, entries) at the claim's (exec_index, event_index), by the walk of step 4"""
    h = header(_get(blocks, _parse_cid(c["child_block_cid"]), "child header"))
    root = amt_get(amt_load(blocks, h.receipts, 0, check_receipt), c["exec_index"])
    return amt_get(amt_load(blocks, root, 3, check_stamped_event), c["event_index"])


def reaches_step_4(blocks, c, trust=None) -> bool:
    """the claim passes steps 1-3 (trust, headers, execution order) and enters verify_receipt_and_event — what the
    mutator's conditions count"""
    try:
        parents = [_parse_cid(s) for s in c["parent_tipset_cids"]]
        child = _parse_cid(c["child_block_cid"])
        if not (_trusted(trust, c["parent_epoch"]) and _trusted(trust, c["child_epoch"])):
            return False
        h = header(_get(blocks, child, "child"))
        if h.parents != parents or h.height != c["child_epoch"] or not parents:
            return False
        if header(_get(blocks, parents[0], "parent")).height != c["parent_epoch"]:
            return False
        order = exec_order(blocks, parents)
        msg = _parse_cid(c["message_cid"])
        return msg in order and order.index(msg) == c["exec_index"]
    except Err:
        return False


# ---- find_matching_events (generator.rs:180-307), offline: the receipt list is the receipts AMT walked in index order ------
def scan(blocks, receipts_root, topic0, topic1, actor=None, lo=0, hi=None):
    """→ (status, has-match list, [(exec_index, event_index, emitter)] in emission order, set of recorded CIDs).
    With a receipt range [lo, hi) (a shard of one tipset: include/ipcfp.h ipcfp_witness_create_subset): the receipt list is
    `amt_for_each` under that range, and has[i - lo] is receipt i."""
    filt = (topic0, topic1)
    try:
        rec = set()
        r_amt = amt_load(blocks, receipts_root, 0, check_receipt, seen=rec)                  # :195-196
        receipts = [(i, v) for i, v in amt_for_each(amt_load(blocks, receipts_root, 0, check_receipt), lo, hi)]  # :199-204 (the RPC list)
        has = [0] * max(0, max((i for i, _ in receipts), default=-1) + 1 - lo)

        def wanted(ev):
            emitter, entries = ev
            if actor is not None and emitter != actor:
                return False                                                                  # :220-224
            log = extract_evm_log(entries)
            return log is not None and matches_log(log[0], filt)                              # :227-231

        # (an events root that many receipts name is walked once per pass: the blocks do not change under a scan, so the walk's
        # events, its Err and the CIDs it records are the same every time)
        walked = {}

        def events_of(root, seen):
            key = (root, seen is not None)
            if key not in walked:
                mine = set() if seen is not None else None
                try:
                    walked[key] = (list(amt_for_each(amt_load(blocks, root, 3, check_stamped_event, seen=mine))), mine)
                except Err as e:
                    walked[key] = (e, mine)
            out, mine = walked[key]
            if seen is not None:
                seen |= mine
            if isinstance(out, Err):
                raise out
            return out

        matching = []
        for i, root in receipts:                                                              # PASS 1 (:209-239)
            if root is None:
                continue
            hit = False
            for _j, ev in events_of(root, None):
                hit = wanted(ev) or hit
            if hit:
                matching.append((i, root))
                has[i - lo] = 1
        triples = []
        for i, root in matching:                                                              # PASS 2 (:242-301)
            if amt_get(r_amt, i) is ABSENT:
                continue                                                                      # :249-251
            for j, ev in events_of(root, rec):
                if wanted(ev):
                    triples.append((i, j, ev[0]))
        return TRUE, has, triples, rec
    except Err as e:
        return e.status, None, None, None


def generate(blocks, parent_cids, child_cid, topic0, topic1, actor=None):
    """generate_event_proof (generator.rs:60-107) offline → (status, [(exec_index, event_index, emitter, message cid)], witness set)"""
    try:
        needed = set()
        receipts_root = header(_get(blocks, child_cid, "child header")).receipts             # :112-119
        txmeta = []
        for p in parent_cids:                                                                 # :122-145
            needed.add(p)
            txmeta.append(header(_get(blocks, p, "parent header")).messages)
        needed |= {child_cid, receipts_root, *txmeta}
        for tx in txmeta:                                                                     # :148-177
            bls, secp = txmeta_roots(_get(blocks, tx, "TxMeta", needed))
            for root in (bls, secp):
                for _ in amt_for_each(amt_load(blocks, root, 0, check_cid_value, seen=needed)):
                    pass
        order = []
        seen = set()
        for tx in txmeta:                                                                     # build_execution_order: no re-hash
            for root in txmeta_roots(_get(blocks, tx, "TxMeta")):
                for _i, c in amt_for_each(amt_load(blocks, root, 0, check_cid_value)):
                    if c not in seen:
                        seen.add(c)
                        order.append(c)
        st, _has, triples, rec = scan(blocks, receipts_root, topic0, topic1, actor)
        if st != TRUE:
            raise Err(st, "find_matching_events")
        proofs = []
        for i, j, em in triples:
            if i >= len(order):
                raise Err(ERR, "Missing message at index")                                    # :244-246
            proofs.append((i, j, em, order[i]))
        needed |= rec
        for c in needed:                                                                      # materialize (witness.rs:43-56)
            _get(blocks, c, "block")
        return TRUE, proofs, needed
    except Err as e:
        return e.status, None, None
