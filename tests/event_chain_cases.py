"""Hand-built tipset pairs for `verify_event_proof` (src/proofs/events/verifier.rs:92-290) and the event scan
(src/proofs/events/generator.rs:180-307), one NAMED case per spelling the synthetic tipset writer never emits:

    CASES[name] = (store, claim, expected status)        META[name] = {"trust", "filter", "scan", "parts", "dropped"}

The expected status is a LITERAL written down from the reference's Rust; tests/pyevents.py (an independent restatement)
must reproduce every literal, and the oracle (CPU) and every route of the engine (GPU) must give it too —
tests/test_event_chain.py, tests/test_gpu_event_chain.py.

`tipset()` writes a minimal valid pair with pyamt's encoders: parent headers → TxMeta → bls / secp `Amtv0<Cid>`, a child
header → receipts `Amtv0` → events `Amt` (v3) roots.  Every part can be re-spelled BEFORE it is hashed (so the chain above
links to the defective block), dropped from the store afterwards, or a claim field edited.

Two kinds of case:
  * witness-level cases (headers, TxMeta, message AMTs, the receipts tree, the claim's strings): a tipset of their own;
  * RECEIPT cases (`RC`: events roots at the table's edges, event sizes, StampedEvent spellings): ONE receipt each, with a
    list of claims against it.  Each runs in a small tipset of its own AND as receipt i of `one_tipset()`, where one batch
    over one witness takes them all down the event table's route.

Statuses as in include/ipcfp.h: 1 TRUE · 2 untrusted parent · 3 untrusted child · 4 parents ≠ · 5 child epoch ≠ · 6 parent
epoch ≠ · 7 message not executed · 8 exec index ≠ · 9 no receipt · 10 no events root · 11 no event · 12 emitter ≠ · 13 no EVM
log · 14 topic count ≠ · 15 topic ≠ · 16 data ≠ · 17 filter · 64 Err (index out of range) · 65 block missing · 66 decode ·
67 TxMeta re-hash · 69 unparsable claim string · 71 `parent_cids[0]` on an empty key."""
import hashlib

import claims as claims_mod
import pyamt
import pystorage
from pyamt import NULL, array, bstr, head, link, raw_root, uint  # noqa: F401  (raw_root: the cases' spelled roots)
from event_spellings import data_bytes, entry, spelling_cases, stamped, text, topic  # noqa: F401  (spelling_cases: re-exported)
from storage_chain_cases import cmap, encode, mutate_field, nint, store_of  # noqa: F401  (store_of: for the tests)

PARENT_EPOCH, CHILD_EPOCH = 4_000_123, 4_000_124
# the four policies of test_event_proofs_adversarial (kind 1: ec_chain_empty, min_epoch, max_epoch) and what each does to a
# claim that is otherwise past step 1
TRUST = {
    "child_outside": ((0, PARENT_EPOCH, PARENT_EPOCH), 3),
    "parent_outside": ((0, CHILD_EPOCH, CHILD_EPOCH + 5), 2),
    "empty_ec_chain": ((1, 0, 10 ** 9), 2),  # (the parent is asked first, verifier.rs:134)
    "both_inside": ((0, PARENT_EPOCH, CHILD_EPOCH), None),
}
BAD = b"\xff"  # no DAG-CBOR item
OTHER = pyamt.cid_of(b"some other block")  # a well-formed CID of a block no witness holds


T = [topic(k) for k in range(1, 10)]
FILTER = (T[0], T[1])        # what most planted events carry in topics 0 and 1
OTHER_FILTER = (T[0], T[2])  # what "B d of …" carries; matches none of the base tipset's planted events but one


def cid_str(cid: bytes) -> str:
    return pystorage.cid_to_string(cid)


def hex0x(b: bytes) -> str:
    return "0x" + bytes(b).hex()


def M(tag) -> bytes:
    """the CID of message `tag` (the message blocks themselves are never in a witness: the verifier reads none)"""
    return pyamt.cid_of(b"message %s" % str(tag).encode())


def log_fields(ev_bytes: bytes) -> dict:
    """the claim's event_data as generate_event_proof writes it (generator.rs:274-282) — through tests/claims.py's
    extract_evm_log, which is thereby held to every literal of a good spelling"""
    em, topics, data = claims_mod.extract_evm_log(ev_bytes)
    return {"emitter": em, "topics": [hex0x(t) for t in topics], "data": hex0x(data)}


def good_event(emitter, topics=(0, 1), n_data=40) -> bytes:
    return stamped(emitter, [entry(f"t{k + 1}", T[t]) for k, t in enumerate(topics)] + [entry("d", data_bytes(n_data, emitter & 0xFF))])


# ---- AMT roots the writer cannot lie about ------------------------------------------------------------------------------------
def events_root(store, events: dict, bw=5, **kw) -> bytes:
    return pyamt.build_amt(store, events, version=3, bit_width=bw, **kw)


def amt_children(store, root: bytes):
    """the CIDs the root node of an AMT root block links to"""
    t = pystorage.decode(store.blocks[root])
    return [x.cid for x in t[-1][1]]


# ---- the tipset pair ----------------------------------------------------------------------------------------------------------
def default_msgs():
    """two parent blocks; parent 1 repeats a message of parent 0 → execution order m0 m1 m2 m3 m4 m5"""
    return [([M(0), M(1), M(2)], [M(3)]), ([M(1), M(4)], [M(5)])]


def first_seen(msgs):
    out = []
    for bls, secp in msgs:
        for c in bls + secp:
            if c not in out:
                out.append(c)
    return out


BASE_EVENTS = {0: stamped(1000, [entry("topics", T[0] + T[1]), entry("data", b"\xaa" * 5)]),  # Case A, matches FILTER
               1: good_event(1001),                                                               # Case B, matches FILTER
               2: good_event(1001, topics=(0, 2, 3))}                                             # Case B, matches OTHER_FILTER
NOT_A_LOG = stamped(1003, [entry("d", b"\x01\x02\x03")])


def default_receipts(n):
    """receipt 1 has no events root, 2 the three BASE_EVENTS, 3 one event that is no EVM log, every other one good event"""
    out = {}
    for i in range(n):
        if i == 1:
            out[i] = lambda st: pyamt.receipt()
        elif i == 2:
            out[i] = lambda st: pyamt.receipt(events_root=events_root(st, BASE_EVENTS))
        elif i == 3:
            out[i] = lambda st: pyamt.receipt(events_root=events_root(st, {0: NOT_A_LOG}))
        else:
            out[i] = (lambda i: lambda st: pyamt.receipt(events_root=events_root(st, {0: good_event(2000 + i)})))(i)
    return out


# what a scan of the default tipset finds: (exec_index, event_index, emitter) in emission order
BASE_SCAN = {(FILTER, None): [(0, 0, 2000), (2, 0, 1000), (2, 1, 1001), (4, 0, 2004), (5, 0, 2005)],
             (FILTER, 1001): [(2, 1, 1001)],
             (OTHER_FILTER, None): [(2, 2, 1001)]}


def header_fields(parents, height, receipts, messages, salt=0):
    return [bstr(b"\x00\xe8\x07"), array([bstr(b"vrf")]), NULL, array([]), array([]), array([link(p) for p in parents]),
            bstr(b"\x00\x01"), uint(height) if height >= 0 else nint(height), link(pyamt.cid_of(b"state root")), link(receipts),
            link(messages), NULL, uint(1_700_000_000 + salt), NULL, uint(0), bstr(b"\x00\x64")]


def tipset(*, msgs=None, receipts=None, salt=0, at=(2, 1), message=None, child_header=None, parent_header=None, txmeta=None,
           msg_amt=None, receipts_amt=None, drop=(), edit=None, parent_epoch=PARENT_EPOCH, child_epoch=CHILD_EPOCH, event=None):
    """A valid tipset pair and one claim against it.
    msgs           per parent block ([bls message CIDs], [secp message CIDs])
    receipts       {index: callable(store) → receipt bytes}; default: one per executed message (default_receipts); "good": one
                   per executed message, each with one good event
    at             (exec_index, event_index) the claim names; its message is the one executed there (or `message`), its
                   event_data is lowered from `event` (StampedEvent bytes; default: what default_receipts put there)
    child_header, parent_header(k, ·), txmeta(k, ·)   callable(default encoded fields) → the block's bytes, to re-spell it
    msg_amt        callable(store, parent k, "bls" | "secp", [cids]) → root CID, or None for the default
    receipts_amt   callable(store, {index: receipt bytes}) → root CID
    drop           names of parts ("child", "parent0", "txmeta1", "bls0", "secp1", "receipts") or CIDs, or
                   callable(parts, store) → [CIDs], removed afterwards
    edit           claim fields overwritten at the end: a dict, or callable(finished claim, parts) → dict
    → (store, claim, parts)"""
    st = pyamt.Store()
    msgs = default_msgs() if msgs is None else msgs
    order = first_seen(msgs)
    grand = pyamt.cid_of(b"grandparent header")
    parts = {"parents": [], "txmeta": [], "order": order, "dropped": []}
    for k, (bls, secp) in enumerate(msgs):
        roots = []
        for which, cids in (("bls", bls), ("secp", secp)):
            r = msg_amt(st, k, which, cids) if msg_amt else None
            if r is None:
                r = pyamt.build_amt(st, {i: link(c) for i, c in enumerate(cids)}, version=0)
            parts[f"{which}{k}"] = r
            roots.append(link(r))
        tx = st.put(txmeta(k, roots) if txmeta else array(roots))
        parts["txmeta"].append(tx)
        parts[f"txmeta{k}"] = tx
        f = header_fields([grand], parent_epoch, pyamt.cid_of(b"older receipts"), tx, salt + k)
        p = st.put(parent_header(k, f) if parent_header else array(f))
        parts["parents"].append(p)
        parts[f"parent{k}"] = p
    all_good = receipts == "good"  # every executed message has a receipt with one good event, emitter 2000 + index
    if all_good:
        receipts = {i: (lambda i: lambda s: pyamt.receipt(events_root=events_root(s, {0: good_event(2000 + i)})))(i) for i in range(len(order))}
    receipts = default_receipts(len(order)) if receipts is None else receipts
    made = {i: (r(st) if callable(r) else r) for i, r in receipts.items()}
    rroot = receipts_amt(st, made) if receipts_amt else pyamt.build_amt(st, made, version=0)
    parts["receipts"] = rroot
    f = header_fields(parts["parents"], child_epoch, rroot, pyamt.cid_of(b"child messages"), salt + 100)
    child = st.put(child_header(f) if child_header else array(f))
    parts["child"] = child
    e, j = at
    if event is None:
        event = good_event(2000 + e) if all_good else BASE_EVENTS[j] if e == 2 and j in BASE_EVENTS else NOT_A_LOG if e == 3 else good_event(2000 + e)
    lf = log_fields(event) if claims_mod.extract_evm_log(event) is not None else {"emitter": pystorage.decode(event)[0], "topics": [], "data": "0x"}
    msg = message if message is not None else (order[e] if e < len(order) else OTHER)
    claim = {"parent_epoch": parent_epoch, "child_epoch": child_epoch, "parent_tipset_cids": [cid_str(p) for p in parts["parents"]],
             "child_block_cid": cid_str(child), "message_cid": cid_str(msg), "exec_index": e, "event_index": j, **lf}
    for d in (drop(parts, st) if callable(drop) else drop):
        c = parts.get(d, d)
        del st.blocks[c]
        parts["dropped"].append(c)
    claim.update(edit(claim, parts) if callable(edit) else (edit or {}))
    return st, claim, parts


CASES = {}  # name → (store, claim, expected status)
META = {}   # name → {"trust", "filter", "scan", "parts", "dropped"}


# The header / TxMeta ladder once more with EVERY header longer than the 8 KB the tipset prologue stages in LDS, so that every
# slot of every route is answered by the prologue's general form (csrc/kernels/tipset_prepare_general.hip): each of these
# cases has a twin `<name>_with_long_headers` with the SAME literal — a header's first field is IgnoredAny and decides nothing.
LONG_HEADERS = "_with_long_headers"
LONG_HEADER_BASES = frozenset("""
    base_true parents_mismatch_order parents_mismatch_count child_epoch_mismatch parent_epoch_mismatch message_not_in_exec
    missing_child_header missing_parent0_header missing_parent1_header missing_txmeta0 missing_txmeta1 missing_bls_root
    missing_secp_root_of_the_last_parent undecodable_txmeta txmeta_as_a_3_tuple txmeta_as_a_1_tuple txmeta_root_null
    txmeta_nonminimal_array_head_rehashes_differently txmeta_of_the_last_parent_rehashes_differently
    two_missing_child_header_and_parents_mismatch two_wrong_child_epoch_and_missing_parent0
    two_missing_parent0_and_parents_mismatch two_wrong_parent_epoch_and_missing_parent1 two_wrong_parent_epoch_and_missing_txmeta
    two_txmeta0_mismatch_and_missing_parent1_header_is_the_header two_txmeta0_mismatch_and_missing_txmeta1
    two_txmeta0_mismatch_and_missing_bls0 two_missing_secp0_and_txmeta1_mismatch two_txmeta_undecodable_and_mismatch_is_the_decode
    child_header_15_tuple child_header_17_tuple parent0_header_15_tuple parent1_header_17_tuple child_parents_holds_a_byte_string
    child_parents_is_not_an_array exec_duplicate_across_parents_first_position exec_first_parent_empty
    undecodable_child_header undecodable_parent0_header undecodable_parent1_header
    two_undecodable_child_header_and_wrong_child_epoch two_undecodable_parent0_and_wrong_parent_epoch""".split())
# (the last five: their undecodable header is the one-byte BAD, which has no first field to lengthen — the OTHER headers are long)


def long_field_0(make, n):
    """header override: the case's own re-spelling `make` (or none) first, then field 0 of the tuple it wrote as a byte
    string of n bytes; a block that is no such tuple stays as it is"""
    def out(f):
        b = make(f) if make else array(f)
        return b[:1] + bstr(bytes(n)) + b[1 + len(f[0]):] if b[1:1 + len(f[0])] == f[0] else b
    return out


def case(name, expect, *, trust=None, filt=None, scan=None, **kw):
    """`scan`: {(filter, actor): expected triples} where the case has a scan answer written down"""
    assert name not in CASES, name
    salt = int.from_bytes(hashlib.sha256(name.encode()).digest()[:3], "big")
    st, claim, parts = tipset(salt=salt, **kw)
    CASES[name] = (st, claim, expect)
    META[name] = {"trust": trust, "filter": filt, "scan": scan, "parts": parts, "dropped": parts["dropped"]}
    if name in LONG_HEADER_BASES:  # the twin, from the same keyword arguments
        ch, ph = kw.get("child_header"), kw.get("parent_header")
        case(name + LONG_HEADERS, expect, trust=trust, filt=filt, scan=scan,
             **{**kw, "child_header": long_field_0(ch, 9000),
                "parent_header": lambda k, f: long_field_0((lambda g: ph(k, g)) if ph else None, 9100 + 16 * k)(f)})


def respell(i, new):
    """header / tuple override: field i replaced by the encoded item `new`"""
    return lambda f: array(f[:i] + [new] + f[i + 1:])


def only(k, fn):
    """parent_header / txmeta override for parent block k alone"""
    return lambda kk, f: fn(f) if kk == k else array(f)


def flip_last(hexstr):
    return hexstr[:-1] + ("0" if hexstr[-1] != "0" else "1")


# ===== the ladder: one case per reachable status, through an otherwise valid chain =========================================
case("base_true", 1, scan=BASE_SCAN)
case("base_true_case_a_event", 1, at=(2, 0))
case("base_true_under_the_matching_filter", 1, filt=FILTER)
case("untrusted_parent", 2, trust=TRUST["parent_outside"][0])
case("untrusted_parent_empty_ec_chain", 2, trust=TRUST["empty_ec_chain"][0])
case("untrusted_child", 3, trust=TRUST["child_outside"][0])
case("trusted_both_epochs_at_the_window_edges", 1, trust=TRUST["both_inside"][0])
case("parents_mismatch_order", 4, edit=lambda c, p: {"parent_tipset_cids": c["parent_tipset_cids"][::-1]})
case("parents_mismatch_count", 4, edit=lambda c, p: {"parent_tipset_cids": c["parent_tipset_cids"][:1]})
case("parents_mismatch_count_one_more", 4, edit=lambda c, p: {"parent_tipset_cids": c["parent_tipset_cids"] + [cid_str(OTHER)]})
case("parents_mismatch_content", 4, edit=lambda c, p: {"parent_tipset_cids": [c["parent_tipset_cids"][0], cid_str(OTHER)]})
case("parents_same_cids_in_multibase_upper_are_equal", 1, edit=lambda c, p: {"parent_tipset_cids": ["B" + s[1:].upper() for s in c["parent_tipset_cids"]]})
case("child_epoch_mismatch", 5, edit={"child_epoch": CHILD_EPOCH + 1})
case("parent_epoch_mismatch", 6, edit={"parent_epoch": PARENT_EPOCH - 1})
case("message_not_in_exec", 7, message=OTHER)
case("exec_index_mismatch", 8, at=(3, 0), message=M(2))
case("no_receipt_hole_at_exec_index", 9, receipts={i: r for i, r in default_receipts(6).items() if i != 2})
case("no_events_root", 10, at=(1, 0))
case("no_event", 11, at=(2, 7), event=BASE_EVENTS[1])
case("wrong_emitter", 12, edit={"emitter": 1002})
case("not_an_evm_log", 13, at=(3, 0))
case("topic_count_one_less", 14, edit=lambda c, p: {"topics": c["topics"][:1]})
case("topic_count_one_more", 14, edit=lambda c, p: {"topics": c["topics"] + [hex0x(T[5])]})
case("topic_last_nibble", 15, edit=lambda c, p: {"topics": [c["topics"][0], flip_last(c["topics"][1])]})
case("topic_first_wrong", 15, edit=lambda c, p: {"topics": [hex0x(T[7]), c["topics"][1]]})
case("data_last_nibble", 16, edit=lambda c, p: {"data": flip_last(c["data"])})
case("data_one_byte_longer", 16, edit=lambda c, p: {"data": c["data"] + "00"})
case("data_one_byte_shorter", 16, edit=lambda c, p: {"data": c["data"][:-2]})
case("filter_does_not_match", 17, filt=OTHER_FILTER)
case("filter_needs_two_topics", 17, filt=(T[0], bytes(32)), receipts={**default_receipts(6), 4: lambda st: pyamt.receipt(events_root=events_root(st, {0: good_event(2004, topics=(0,))}))},
     at=(4, 0), event=good_event(2004, topics=(0,)))
# 64: `events_amt.get(u64::MAX)` is Err(OutOfRange) (pyevents.AMT_MAX_INDEX_IS_U64_MAX_MINUS_1)
case("event_index_u64_max_is_out_of_range", 64, edit={"event_index": (1 << 64) - 1})
# 65: every block the verifier fetches
case("missing_child_header", 65, drop=["child"])
case("missing_parent0_header", 65, drop=["parent0"])
case("missing_parent1_header", 65, drop=["parent1"])
case("missing_txmeta0", 65, drop=["txmeta0"])
case("missing_txmeta1", 65, drop=["txmeta1"])
case("missing_bls_root", 65, drop=["bls0"])
case("missing_secp_root_of_the_last_parent", 65, drop=["secp1"])
NINE = [M(f"n{i}") for i in range(9)]  # 9 messages: an Amtv0 of height 1 with two leaves
NINE_MSGS = [(NINE, [M(3)]), ([M(4)], [])]
case("missing_message_amt_node", 65, msgs=NINE_MSGS, at=(0, 0), drop=lambda p, st: [amt_children(st, p["bls0"])[1]])
case("missing_receipts_root", 65, drop=["receipts"])
case("missing_receipts_node_on_the_path", 65, msgs=NINE_MSGS, at=(0, 0), drop=lambda p, st: [amt_children(st, p["receipts"])[0]])
case("missing_receipts_node_off_the_path_is_not_read", 1, msgs=NINE_MSGS, at=(0, 0), drop=lambda p, st: [amt_children(st, p["receipts"])[1]])


def _events_at_2(make_root):
    """default receipts with receipt 2's events root made by callable(store) → CID"""
    return {**default_receipts(6), 2: lambda st: pyamt.receipt(events_root=make_root(st))}


def _dropped_root(st, events, **kw):
    r = events_root(st, events, **kw)
    del st.blocks[r]
    return r


def _root_without_child(st, events, which, **kw):
    r = events_root(st, events, **kw)
    del st.blocks[amt_children(st, r)[which]]
    return r


DEEP = {0: good_event(3000), 1: good_event(3001), 2: good_event(3002), 3: good_event(3003)}  # bit width 1: height 1, two leaves
case("missing_events_root", 65, receipts=_events_at_2(lambda st: _dropped_root(st, BASE_EVENTS)))
case("missing_events_node_on_the_path", 65, receipts=_events_at_2(lambda st: _root_without_child(st, DEEP, 1, bw=1)), at=(2, 2), event=DEEP[2])
case("missing_events_node_off_the_path_is_not_read", 1, receipts=_events_at_2(lambda st: _root_without_child(st, DEEP, 0, bw=1)), at=(2, 2), event=DEEP[2])
case("events_amt_of_height_1", 1, receipts=_events_at_2(lambda st: events_root(st, DEEP, bw=1)), at=(2, 3), event=DEEP[3])
# 66: every decode site
case("undecodable_child_header", 66, child_header=lambda f: BAD + b"child")
case("undecodable_parent0_header", 66, parent_header=only(0, lambda f: BAD + b"parent 0"))
case("undecodable_parent1_header", 66, parent_header=only(1, lambda f: BAD + b"parent 1"))
case("undecodable_txmeta", 66, txmeta=only(0, lambda f: BAD + b"txmeta"))
case("txmeta_as_a_3_tuple", 66, txmeta=only(1, lambda f: array(f + [NULL])))
case("txmeta_as_a_1_tuple", 66, txmeta=only(0, lambda f: array(f[:1])))
case("txmeta_root_null", 66, txmeta=only(0, lambda f: array([f[0], NULL])))
case("undecodable_message_amt_root", 66, msg_amt=lambda st, k, w, c: st.put(BAD + b"bls") if (k, w) == (0, "bls") else None)
case("message_amt_root_is_a_v3_root", 66, msg_amt=lambda st, k, w, c: pyamt.build_amt(st, {0: link(c[0])}, version=3, bit_width=3) if (k, w) == (1, "secp") else None)
case("message_amt_value_is_not_a_cid", 66, msg_amt=lambda st, k, w, c: pyamt.build_amt(st, {0: link(c[0]), 1: bstr(c[1])}, version=0) if (k, w) == (1, "bls") else None)
case("message_amt_value_is_null", 66, msg_amt=lambda st, k, w, c: pyamt.build_amt(st, {0: NULL}, version=0) if (k, w) == (0, "secp") else None)


def _bad_second_leaf(st, cids):
    """9 entries: the second leaf (index 8) holds an int where a CID belongs"""
    return pyamt.build_amt(st, {**{i: link(c) for i, c in enumerate(cids[:8])}, 8: uint(7)}, version=0)


case("undecodable_message_amt_node", 66, msgs=NINE_MSGS, at=(0, 0), msg_amt=lambda st, k, w, c: _bad_second_leaf(st, c) if (k, w) == (0, "bls") else None)
case("undecodable_receipts_root", 66, receipts_amt=lambda st, made: st.put(BAD + b"receipts"))
case("receipts_root_is_a_v3_root", 66, receipts_amt=lambda st, made: pyamt.build_amt(st, made, version=3, bit_width=3))
RECEIPT_3 = array([uint(0), bstr(b""), uint(1000)])
case("receipt_of_3_fields_at_the_claimed_index", 66, receipts={**default_receipts(6), 2: RECEIPT_3})
case("receipt_of_3_fields_at_a_sibling_in_the_same_node", 66, receipts={**default_receipts(6), 5: RECEIPT_3})
case("receipt_of_5_fields_at_a_sibling", 66, receipts={**default_receipts(6), 0: array([uint(0), bstr(b""), uint(1), NULL, uint(0)])})
case("receipt_exit_code_2_pow_32_at_a_sibling", 66, receipts={**default_receipts(6), 4: array([uint(1 << 32), bstr(b""), uint(1), NULL])})
case("receipt_events_root_is_a_byte_string", 66, receipts={**default_receipts(6), 2: array([uint(0), bstr(b""), uint(1), bstr(OTHER)])})


def _nine_receipts(bad_at):
    r = default_receipts(10)
    r[bad_at] = RECEIPT_3
    return r


case("undecodable_receipts_node_on_the_path", 66, msgs=NINE_MSGS, at=(0, 0), receipts=_nine_receipts(7))
case("undecodable_receipts_node_off_the_path_is_not_read", 1, msgs=NINE_MSGS, at=(0, 0), receipts=_nine_receipts(8))
case("undecodable_events_root", 66, receipts=_events_at_2(lambda st: st.put(BAD + b"events")))
case("events_root_is_the_receipts_shape_a_v0_3_tuple", 66, receipts=_events_at_2(lambda st: pyamt.build_amt(st, BASE_EVENTS, version=0)))
case("events_root_names_a_receipts_root", 66, receipts=_events_at_2(lambda st: pyamt.build_amt(st, {0: pyamt.receipt()}, version=0)))
case("events_root_names_a_header", 66, receipts=_events_at_2(lambda st: st.put(array(header_fields([OTHER], 5, OTHER, OTHER)))))


def _deep_with_bad_leaf(st, which):
    ev = dict(DEEP)
    ev[which] = array([uint(3000), uint(7)])  # an ActorEvent that is no array
    return events_root(st, ev, bw=1)


case("undecodable_events_node_on_the_path", 66, receipts=_events_at_2(lambda st: _deep_with_bad_leaf(st, 3)), at=(2, 2), event=DEEP[2])
case("undecodable_events_node_off_the_path_is_not_read", 1, receipts=_events_at_2(lambda st: _deep_with_bad_leaf(st, 0)), at=(2, 2), event=DEEP[2])
# 67: the TxMeta decodes, its canonical re-encoding hashes to another CID (utils.rs:64-72)
case("txmeta_nonminimal_array_head_rehashes_differently", 67, txmeta=only(0, lambda f: b"\x98\x02" + b"".join(f)))
case("txmeta_of_the_last_parent_rehashes_differently", 67, txmeta=only(1, lambda f: b"\x98\x02" + b"".join(f)))
# 69: each claim string; a parent or child string is met in verify_trust_anchors, before trust and before any block
case("claim_parent0_garbage", 69, edit=lambda c, p: {"parent_tipset_cids": ["garbage", c["parent_tipset_cids"][1]]})
case("claim_parent1_garbage", 69, edit=lambda c, p: {"parent_tipset_cids": [c["parent_tipset_cids"][0], ""]})
case("claim_child_garbage", 69, edit={"child_block_cid": "bafy-not-base32"})
case("claim_message_garbage", 69, edit={"message_cid": "garbage"})
case("claim_parent_garbage_before_trust", 69, trust=TRUST["parent_outside"][0], edit=lambda c, p: {"parent_tipset_cids": ["garbage"]})
case("claim_child_garbage_before_trust", 69, trust=TRUST["empty_ec_chain"][0], edit={"child_block_cid": "garbage"})
case("claim_child_garbage_before_any_block", 69, drop=["child", "parent0"], edit={"child_block_cid": "garbage"})
case("claim_message_in_multibase_upper_is_the_same_cid", 1, edit=lambda c, p: {"message_cid": "B" + c["message_cid"][1:].upper()})
case("claim_child_in_base16_is_the_same_cid", 1, edit=lambda c, p: {"child_block_cid": "f" + p["child"].hex()})
# 71: `parent_cids[0]` on an empty key — both the header's and the claim's `parents` empty, the epochs right
case("empty_parents_on_both_sides", 71, child_header=respell(5, array([])), edit={"parent_tipset_cids": []})
case("empty_parents_in_the_claim_only", 4, edit={"parent_tipset_cids": []})
case("empty_parents_on_both_sides_wrong_child_epoch", 5, child_header=respell(5, array([])), edit={"parent_tipset_cids": [], "child_epoch": 7})
# hex compares: eq_ignore_ascii_case over "0x" + hex
case("claim_topics_upper_case", 1, edit=lambda c, p: {"topics": ["0x" + t[2:].upper() for t in c["topics"]]})
case("claim_topics_0X_prefix", 1, edit=lambda c, p: {"topics": ["0X" + t[2:] for t in c["topics"]]})
case("claim_topic_without_0x", 15, edit=lambda c, p: {"topics": [c["topics"][0], c["topics"][1][2:]]})
case("claim_data_upper_case", 1, edit=lambda c, p: {"data": "0x" + c["data"][2:].upper()})
case("claim_data_0X_prefix", 1, edit=lambda c, p: {"data": "0X" + c["data"][2:]})
case("claim_data_without_0x", 16, edit=lambda c, p: {"data": c["data"][2:]})
case("claim_data_with_a_non_hex_digit", 16, edit=lambda c, p: {"data": c["data"][:-1] + "g"})

# ===== two defects in one chain: the earlier step's status comes out =====================================================
# steps: parent strings → child string → parent trust → child trust → child header → parents compare → child epoch →
#   parents[0] header → parent epoch → EVERY parent header → per parent (TxMeta fetch, decode, re-hash, bls walk, secp walk) →
#   message string → position → index → child header → receipts root → receipt → events_root → events root → event →
#   emitter → log → topic count → topics → data → filter
WIN_BOTH_OUT = (0, CHILD_EPOCH + 1, CHILD_EPOCH + 9)
case("two_garbage_parent_and_garbage_child", 69, edit=lambda c, p: {"parent_tipset_cids": ["x"], "child_block_cid": "y"})
case("two_garbage_child_and_untrusted_parent", 69, trust=WIN_BOTH_OUT, edit={"child_block_cid": "garbage"})
case("two_untrusted_parent_and_untrusted_child", 2, trust=WIN_BOTH_OUT)
case("two_untrusted_child_and_missing_child_header", 3, trust=TRUST["child_outside"][0], drop=["child"])
case("two_missing_child_header_and_parents_mismatch", 65, drop=["child"], edit=lambda c, p: {"parent_tipset_cids": c["parent_tipset_cids"][:1]})
case("two_undecodable_child_header_and_wrong_child_epoch", 66, child_header=lambda f: BAD + b"two", edit={"child_epoch": 3})
case("two_parents_mismatch_and_wrong_child_epoch", 4, edit=lambda c, p: {"parent_tipset_cids": c["parent_tipset_cids"][::-1], "child_epoch": 3})
case("two_wrong_child_epoch_and_missing_parent0", 5, drop=["parent0"], edit={"child_epoch": 3})
case("two_missing_parent0_and_parents_mismatch", 4, drop=["parent0"], edit=lambda c, p: {"parent_tipset_cids": c["parent_tipset_cids"][::-1][:1]})
case("two_missing_parent0_and_wrong_parent_epoch", 65, drop=["parent0"], edit={"parent_epoch": 3})
case("two_undecodable_parent0_and_wrong_parent_epoch", 66, parent_header=only(0, lambda f: BAD + b"p0"), edit={"parent_epoch": 3})
case("two_wrong_parent_epoch_and_missing_parent1", 6, drop=["parent1"], edit={"parent_epoch": 3})
case("two_wrong_parent_epoch_and_missing_txmeta", 6, drop=["txmeta0"], edit={"parent_epoch": 3})
# utils.rs:20-27 reads EVERY parent header before :56 opens the first TxMeta
case("two_txmeta0_mismatch_and_missing_parent1_header_is_the_header", 65, txmeta=only(0, lambda f: b"\x98\x02" + b"".join(f)), drop=["parent1"])
case("two_txmeta0_mismatch_and_missing_txmeta1", 67, txmeta=only(0, lambda f: b"\x98\x02" + b"".join(f)), drop=["txmeta1"])
case("two_txmeta0_mismatch_and_missing_bls0", 67, txmeta=only(0, lambda f: b"\x98\x02" + b"".join(f)), drop=["bls0"])
case("two_missing_secp0_and_txmeta1_mismatch", 65, txmeta=only(1, lambda f: b"\x98\x02" + b"".join(f)), drop=["secp0"])
case("two_txmeta_undecodable_and_mismatch_is_the_decode", 66, txmeta=only(0, lambda f: b"\x98\x03" + b"".join(f) + NULL))
# verifier.rs:190-193: `message_cid` is parsed only after reconstruct_execution_order returned
case("two_txmeta_mismatch_and_garbage_message", 67, txmeta=only(1, lambda f: b"\x98\x02" + b"".join(f)), edit={"message_cid": "garbage"})
case("two_missing_bls_root_and_garbage_message", 65, drop=["bls1"], edit={"message_cid": "garbage"})
case("two_missing_parent1_and_garbage_message", 65, drop=["parent1"], edit={"message_cid": "garbage"})
case("two_garbage_message_and_missing_receipts_root", 69, drop=["receipts"], edit={"message_cid": "garbage"})
case("two_message_not_in_exec_and_missing_receipts_root", 7, message=OTHER, drop=["receipts"])
case("two_wrong_exec_index_and_missing_receipts_root", 8, at=(3, 0), message=M(2), drop=["receipts"])
case("two_missing_receipts_root_and_wrong_emitter", 65, drop=["receipts"], edit={"emitter": 5})
case("two_absent_receipt_and_wrong_emitter", 9, receipts={i: r for i, r in default_receipts(6).items() if i != 2}, edit={"emitter": 5})
case("two_no_events_root_and_wrong_emitter", 10, at=(1, 0), edit={"emitter": 5})
case("two_missing_events_root_and_wrong_emitter", 65, receipts=_events_at_2(lambda st: _dropped_root(st, BASE_EVENTS)), edit={"emitter": 5})
case("two_no_event_and_wrong_emitter", 11, at=(2, 7), event=BASE_EVENTS[1], edit={"emitter": 5})
case("two_index_out_of_range_and_missing_events_root_is_the_block", 65, receipts=_events_at_2(lambda st: _dropped_root(st, BASE_EVENTS)), edit={"event_index": (1 << 64) - 1})
case("two_wrong_emitter_and_not_an_evm_log", 12, at=(3, 0), edit={"emitter": 5})
case("two_not_an_evm_log_and_topic_count", 13, at=(3, 0), edit={"topics": [hex0x(T[0])]})
case("two_topic_count_and_wrong_topic", 14, edit=lambda c, p: {"topics": [hex0x(T[8])]})
case("two_wrong_topic_and_wrong_data", 15, edit=lambda c, p: {"topics": [c["topics"][0], hex0x(T[8])], "data": "0x"})
case("two_wrong_data_and_filter", 16, filt=OTHER_FILTER, edit={"data": "0x00"})
case("two_wrong_emitter_and_filter", 12, filt=OTHER_FILTER, edit={"emitter": 5})

# ===== execution order (utils.rs:53-91): ONE `seen` set, first-seen order, bls before secp, parents in key order ===========
A, B_, C_, D_ = M("a"), M("b"), M("c"), M("d")
DUP_BLS = [([A, B_, A, C_], [D_])]
case("exec_duplicate_within_bls_first_position", 1, msgs=DUP_BLS, at=(0, 0), message=A, receipts="good")
case("exec_duplicate_within_bls_later_position", 8, msgs=DUP_BLS, at=(2, 0), message=A, receipts="good")
case("exec_duplicate_within_bls_the_one_behind_it", 1, msgs=DUP_BLS, at=(2, 0), message=C_, receipts="good")
case("exec_duplicate_within_bls_raw_position_of_the_one_behind", 8, msgs=DUP_BLS, at=(3, 0), message=C_, receipts="good")
DUP_SECP = [([A, B_], [B_, C_])]
case("exec_duplicate_across_bls_and_secp_first_position", 1, msgs=DUP_SECP, at=(1, 0), message=B_, receipts="good")
case("exec_duplicate_across_bls_and_secp_later_position", 8, msgs=DUP_SECP, at=(2, 0), message=B_, receipts="good")
case("exec_duplicate_across_bls_and_secp_the_one_behind_it", 1, msgs=DUP_SECP, at=(2, 0), message=C_, receipts="good")
DUP_PARENTS = [([A, B_], []), ([C_], [A]), ([B_, D_], [])]
case("exec_duplicate_across_parents_first_position", 1, msgs=DUP_PARENTS, at=(0, 0), message=A, receipts="good")
case("exec_duplicate_across_parents_later_position", 8, msgs=DUP_PARENTS, at=(3, 0), message=A, receipts="good")
case("exec_duplicate_across_parents_the_one_behind_both", 1, msgs=DUP_PARENTS, at=(3, 0), message=D_, receipts="good")
case("exec_duplicate_across_parents_position_as_if_deduped_per_parent", 8, msgs=DUP_PARENTS, at=(5, 0), message=D_, receipts="good")
case("exec_message_only_in_the_last_parent", 1, at=(5, 0), receipts="good")
case("exec_secp_comes_after_bls_of_the_same_parent", 1, at=(3, 0), receipts="good")
case("exec_first_parent_empty", 1, msgs=[([], []), ([A], [B_])], at=(1, 0), message=B_, receipts="good")
case("exec_both_amts_empty_everywhere", 7, msgs=[([], []), ([], [])], at=(0, 0), message=A, receipts=default_receipts(2))
for _n in (1, 8, 9, 64, 65):
    _m = [M(f"s{_n}_{i}") for i in range(_n)]
    case(f"exec_message_amt_of_{_n}_entries_last_one", 1, msgs=[(_m, [])], at=(_n - 1, 0), receipts="good")
    case(f"exec_message_amt_of_{_n}_entries_in_secp_behind_one_bls", 1, msgs=[([A], _m)], at=(_n, 0), receipts="good")
SPARSE = [M("sp0"), M("sp1"), M("sp2")]
case("exec_sparse_message_amt_counts_positions_not_indices", 1, msgs=[(SPARSE, [])], at=(2, 0), receipts="good",
     msg_amt=lambda st, k, w, c: pyamt.build_amt(st, {0: link(c[0]), 5: link(c[1]), 70: link(c[2])}, version=0) if w == "bls" else None)
case("exec_sparse_message_amt_index_is_not_the_position", 8, msgs=[(SPARSE, [])], at=(5, 0), message=SPARSE[1], receipts=default_receipts(6),
     msg_amt=lambda st, k, w, c: pyamt.build_amt(st, {0: link(c[0]), 5: link(c[1]), 70: link(c[2])}, version=0) if w == "bls" else None)
case("exec_message_amt_count_lies", 1, at=(2, 0), msg_amt=lambda st, k, w, c: pyamt.build_amt(st, {i: link(x) for i, x in enumerate(c)}, version=0, count=99) if (k, w) == (0, "bls") else None, receipts="good")

# ===== headers (common/decode.rs:100-118) ======================================================================================
case("child_header_15_tuple", 66, child_header=lambda f: array(f[:15]))
case("child_header_17_tuple", 66, child_header=lambda f: array(f + [NULL]))
case("parent0_header_15_tuple", 66, parent_header=only(0, lambda f: array(f[:15])))
case("parent1_header_17_tuple", 66, parent_header=only(1, lambda f: array(f + [NULL])))
case("child_height_minus_1_with_claim_epoch_minus_1", 1, child_epoch=-1)
case("parent_height_minus_1_with_claim_epoch_minus_1", 1, parent_epoch=-1)
case("child_height_2_pow_63", 66, child_header=respell(7, uint(1 << 63)))
case("child_height_i64_max", 5, child_header=respell(7, uint((1 << 63) - 1)))
case("child_height_minus_2_pow_63", 5, child_header=respell(7, head(1, (1 << 63) - 1)))
case("child_height_below_i64", 66, child_header=respell(7, head(1, 1 << 63)))
case("parent1_height_2_pow_63_is_read_by_the_execution_order", 66, parent_header=only(1, respell(7, uint(1 << 63))))
case("parent1_height_differs_and_nobody_compares_it", 1, parent_header=only(1, respell(7, uint(5))))
case("child_parents_holds_a_byte_string", 66, child_header=lambda f: array(f[:5] + [array([bstr(b"\x00" + OTHER)])] + f[6:]),
     edit={"parent_tipset_cids": [cid_str(OTHER)]})
case("child_parents_is_not_an_array", 66, child_header=respell(5, NULL))
case("child_messages_null", 66, child_header=respell(10, NULL))
case("child_timestamp_negative", 66, child_header=respell(12, nint(-1)))
case("child_fork_signaling_a_text", 66, child_header=respell(14, text("0")))
NESTED = array([array([uint(1), cmap([("a", array([NULL, bstr(b"x")]))])]), cmap([("k", link(OTHER))])])
case("ignored_fields_hold_nested_arrays_and_maps", 1, child_header=lambda f: array([NESTED, NESTED, f[2], NESTED, NESTED] + f[5:6] + [NESTED] + f[7:11] + [NESTED, f[12], NESTED, f[14], NESTED]),
     parent_header=lambda k, f: array([NESTED] + f[1:15] + [NESTED]))
case("ignored_field_holds_an_undecodable_item", 66, child_header=respell(0, b"\xc1\x00"))
# the tipset prologue stages 8 KB of a header; a longer one is legal (the first field is IgnoredAny)
case("headers_longer_than_the_prologue_stage", 1, child_header=respell(0, bstr(bytes(9000))), parent_header=only(0, respell(0, bstr(bytes(9100)))))
# … and a TxMeta beyond it: what is found under the TxMeta's CID is the pair and 9000 more bytes, so the decode fails at its
# end (utils.rs:61) — in the LDS prologue the header fit and the TxMeta did not
LONG_TXMETA = lambda f: array(f) + bytes(9000)  # noqa: E731
case("txmeta0_with_a_trailer_longer_than_the_prologue_stage", 66, txmeta=only(0, LONG_TXMETA))
case("txmeta1_with_a_trailer_longer_than_the_prologue_stage", 66, txmeta=only(1, LONG_TXMETA))
# (headers come before any TxMeta: utils.rs:20-27)
case("two_txmeta0_trailer_longer_than_the_prologue_stage_and_missing_parent1_header", 65, txmeta=only(0, LONG_TXMETA), drop=["parent1"])
case("header_trailing_byte", 66, child_header=lambda f: array(f) + b"\x00")

# ===== receipts ==================================================================================================================
case("receipt_exec_index_beyond_the_receipts", 9, receipts=default_receipts(4), at=(5, 0))
case("receipt_exec_index_beyond_the_root_s_height", 9, msgs=NINE_MSGS, receipts=default_receipts(8), at=(8, 0))
for _n in (1, 8, 9, 64, 65):
    _m = [M(f"r{_n}_{i}") for i in range(_n)]
    case(f"receipts_{_n}_last_one", 1, msgs=[(_m, [])], at=(_n - 1, 0))
case("receipts_count_says_100", 1, receipts_amt=lambda st, made: pyamt.build_amt(st, made, version=0, count=100))
case("receipts_count_says_0", 1, receipts_amt=lambda st, made: pyamt.build_amt(st, made, version=0, count=0))
case("receipts_count_lies_over_two_levels", 1, msgs=NINE_MSGS, at=(8, 0), receipts_amt=lambda st, made: pyamt.build_amt(st, made, version=0, count=3))
case("receipts_count_spelled_in_two_bytes", 1, receipts_amt=lambda st, made: raw_root(st, [made[i] for i in sorted(made)], b"\x3f", count=b"\x19\x00\x06", v0=True))
case("receipts_sparse_hole_then_the_claimed_one", 1, receipts={i: r for i, r in default_receipts(6).items() if i not in (0, 1)})
case("receipts_height_1_with_a_single_leaf", 1, receipts_amt=lambda st, made: pyamt.build_amt(st, made, version=0, height=1))
case("receipt_return_data_and_exit_code_are_not_compared", 1,
     receipts={**default_receipts(6), 2: lambda st: pyamt.receipt(exit_code=(1 << 32) - 1, ret=bytes(range(200)), gas=(1 << 64) - 1, events_root=events_root(st, BASE_EVENTS))})


# ===== RECEIPT cases: one receipt, a list of claims against it ===================================================================
RC = []  # (name, callable(store) → receipt bytes, [(claim name, claim fields, expected status)], {dropped CIDs})


def rcase(name, make_root, claim_list):
    """make_root: callable(store) → events root CID (it may delete blocks again).  claim fields: event_index, emitter, topics,
    data (strings as the claim holds them)"""
    assert all(n != name for n, *_ in RC), name
    RC.append((name, make_root, claim_list))


def at_index(j, ev_bytes, **over):
    """the honest claim for the event at index j, fields overridden"""
    f = {"event_index": j, **log_fields(ev_bytes)}
    f.update(over)
    return f


def perturbed(j, ev_bytes):
    """[(tag, fields, expected)]: the honest claim of a good spelling and the four ways to get it wrong"""
    f = at_index(j, ev_bytes)
    out = [("honest", f, 1), ("emitter", {**f, "emitter": (f["emitter"] + 1) & ((1 << 64) - 1)}, 12)]
    t, d = f["topics"], f["data"]
    out.append(("one_topic_less", {**f, "topics": t[:-1]}, 14) if t else ("one_topic_more", {**f, "topics": [hex0x(T[0])]}, 14))
    if t:
        out.append(("last_topic", {**f, "topics": t[:-1] + [flip_last(t[-1])]}, 15))
    out.append(("data_one_byte_longer", {**f, "data": d + "5a"}, 16))
    if len(d) > 2:
        out.append(("last_data_byte", {**f, "data": flip_last(d)}, 16))
    return out


SIB = good_event(4000, topics=(0, 1), n_data=3)  # the well-formed neighbour of a case's event


def _leaf(bw, events, **kw):
    return lambda st: events_root(st, events, bw=bw, **kw)


# --- leaf roots of bit width 1-8, from 6 up with the highest index present; the index one past the node --------------------
for _bw in range(1, 9):
    _w = 1 << _bw
    _ev = {0: good_event(5000 + _bw), _w - 1: good_event(5100 + _bw, topics=(0, 2), n_data=33)}
    rcase(f"leaf_root_bit_width_{_bw}", _leaf(_bw, _ev), [
        ("first", at_index(0, _ev[0]), 1), ("highest", at_index(_w - 1, _ev[_w - 1]), 1),
        ("highest_wrong_data", at_index(_w - 1, _ev[_w - 1], data="0x"), 16),
        ("one_past_the_node", at_index(_w, _ev[0]), 11), ("clear_bit", at_index(1, _ev[0]), 11 if _bw > 1 else 1)][: 5 if _bw > 1 else 4])
FULL6 = {i: good_event(5200 + i, n_data=i) for i in range(64)}
rcase("leaf_root_bit_width_6_all_64_present", _leaf(6, FULL6), [(f"index_{i}", at_index(i, FULL6[i]), 1) for i in (0, 31, 32, 62, 63)] + [("index_64", at_index(64, FULL6[0]), 11)])
# --- event_index at the edges of the table's 64-bit mask and of u64 -----------------------------------------------------------
EDGE6 = {0: good_event(5300), 31: good_event(5331), 32: good_event(5332), 63: good_event(5363)}
rcase("event_index_edges_bit_width_6", _leaf(6, EDGE6), [(f"index_{i}", at_index(i, EDGE6[i]), 1) for i in (0, 31, 32, 63)] + [
    ("index_64", at_index(64, EDGE6[0]), 11), ("index_2_pow_32", at_index(1 << 32, EDGE6[0]), 11),
    ("index_2_pow_32_plus_31", at_index((1 << 32) + 31, EDGE6[31]), 11), ("index_2_pow_63", at_index(1 << 63, EDGE6[0]), 11),
    ("index_2_pow_64_minus_2", at_index((1 << 64) - 2, EDGE6[0]), 11), ("index_2_pow_64_minus_1", at_index((1 << 64) - 1, EDGE6[0]), 64)])
EDGE5 = {0: good_event(5400), 31: good_event(5431)}
rcase("event_index_edges_bit_width_5", _leaf(5, EDGE5), [("index_31", at_index(31, EDGE5[31]), 1), ("index_32", at_index(32, EDGE5[0]), 11),
                                                        ("index_63", at_index(63, EDGE5[31]), 11), ("index_64", at_index(64, EDGE5[0]), 11),
                                                        ("index_2_pow_64_minus_1", at_index((1 << 64) - 1, EDGE5[0]), 64)])
# --- height 1 -----------------------------------------------------------------------------------------------------------------------
H1 = {0: good_event(5500), 1: good_event(5501, n_data=31)}
rcase("height_1_with_one_child", _leaf(3, H1, height=1), [("index_1", at_index(1, H1[1]), 1), ("index_8_in_a_clear_subtree", at_index(8, H1[0]), 11),
                                                          ("index_64_past_the_height", at_index(64, H1[0]), 11)])
H1B = {0: good_event(5510), 9: good_event(5519, n_data=32)}
rcase("height_1_with_a_missing_child", lambda st: _root_without_child(st, H1B, 1, bw=3), [
    ("in_the_child_that_is_there", at_index(0, H1B[0]), 1), ("in_the_missing_child", at_index(9, H1B[9]), 65),
    ("in_a_clear_subtree", at_index(17, H1B[0]), 11)])
# --- `count`: immediate, one byte, two bytes, lying (pyevents.AMT_COUNT_IS_NOT_CHECKED) ----------------------------------------------
CNT = {0: good_event(5600), 1: good_event(5601, topics=(0, 1, 2), n_data=32)}


def _counted(count, **kw):
    return lambda st: raw_root(st, [CNT[0], CNT[1]], b"\x03\x00\x00\x00", count=count, **kw)


for _tag, _cnt in (("immediate", uint(2)), ("one_byte", b"\x18\x02"), ("two_bytes", b"\x19\x00\x02"), ("eight_bytes", b"\x1b" + (2).to_bytes(8, "big")),
                   ("lying_0", uint(0)), ("lying_1", uint(1)), ("lying_1000", uint(1000))):
    rcase(f"count_{_tag}", _counted(_cnt), [("index_0", at_index(0, CNT[0]), 1), ("index_1", at_index(1, CNT[1]), 1), ("index_2", at_index(2, CNT[0]), 11)])
rcase("count_negative", _counted(nint(-1)), [("index_0", at_index(0, CNT[0]), 66)])
rcase("height_spelled_in_one_byte", lambda st: st.put(array([uint(5), b"\x18\x00", uint(2), array([bstr(b"\x03\x00\x00\x00"), array([]), array([CNT[0], CNT[1]])])])),
      [("index_1", at_index(1, CNT[1]), 1)])
rcase("bit_width_spelled_in_one_byte", lambda st: st.put(array([b"\x18\x05", uint(0), uint(2), array([bstr(b"\x03\x00\x00\x00"), array([]), array([CNT[0], CNT[1]])])])),
      [("index_1", at_index(1, CNT[1]), 1)])
rcase("values_array_head_spelled_in_one_byte", lambda st: st.put(array([uint(5), uint(0), uint(2), array([bstr(b"\x03\x00\x00\x00"), array([]), b"\x98\x02" + CNT[0] + CNT[1]])])),
      [("index_0", at_index(0, CNT[0]), 1), ("index_1", at_index(1, CNT[1]), 1)])
# --- a bitmap whose length or popcount disagrees; links where none belong; a trailing byte -------------------------------------
rcase("bitmap_one_byte_short", lambda st: raw_root(st, [CNT[0], CNT[1]], b"\x03\x00\x00"), [("index_0", at_index(0, CNT[0]), 66), ("index_40", at_index(40, CNT[0]), 66)])
rcase("bitmap_one_byte_long", lambda st: raw_root(st, [CNT[0], CNT[1]], b"\x03\x00\x00\x00\x00"), [("index_0", at_index(0, CNT[0]), 66)])
rcase("bitmap_popcount_above_the_values", lambda st: raw_root(st, [CNT[0], CNT[1]], b"\x07\x00\x00\x00"), [("index_0", at_index(0, CNT[0]), 66), ("index_5_clear", at_index(5, CNT[0]), 66)])
rcase("bitmap_popcount_below_the_values", lambda st: raw_root(st, [CNT[0], CNT[1]], b"\x01\x00\x00\x00"), [("index_0", at_index(0, CNT[0]), 66)])
rcase("bitmap_empty_and_no_values", lambda st: raw_root(st, [], b"\x00\x00\x00\x00"), [("index_0", at_index(0, CNT[0]), 11)])
rcase("bitmap_bits_beyond_the_width_are_ignored", lambda st: raw_root(st, [CNT[0]], b"\xf1", bw=2), [("index_0", at_index(0, CNT[0]), 1), ("index_4", at_index(4, CNT[0]), 11)])
# (pyevents.AMT_LINKS_AT_HEIGHT_0_ARE_AN_ERR_OF_THE_WALK: an index the height cannot hold is None before the node is looked at)
rcase("links_in_a_height_0_root", lambda st: raw_root(st, [], b"\x01\x00\x00\x00", links=[OTHER]), [("index_0", at_index(0, CNT[0]), 66), ("index_3_clear", at_index(3, CNT[0]), 66),
                                                                                                    ("index_32_past_the_height", at_index(32, CNT[0]), 11)])
rcase("links_and_values_in_one_node", lambda st: raw_root(st, [CNT[0]], b"\x01\x00\x00\x00", links=[OTHER]), [("index_0", at_index(0, CNT[0]), 66)])
rcase("trailing_byte_after_the_root", lambda st: raw_root(st, [CNT[0], CNT[1]], b"\x03\x00\x00\x00", trailer=b"\x00"), [("index_0", at_index(0, CNT[0]), 66)])
rcase("root_of_3_fields", lambda st: st.put(array([uint(0), uint(1), array([bstr(b"\x01\x00\x00\x00"), array([]), array([CNT[0]])])])), [("index_0", at_index(0, CNT[0]), 66)])
rcase("root_of_5_fields", lambda st: st.put(array([uint(5), uint(0), uint(1), array([bstr(b"\x01\x00\x00\x00"), array([]), array([CNT[0]])]), NULL])), [("index_0", at_index(0, CNT[0]), 66)])
rcase("events_root_missing", lambda st: _dropped_root(st, {0: good_event(5700)}), [("index_0", at_index(0, good_event(5700)), 65)])


# --- event size: the table's 16-bit fields ---------------------------------------------------------------------------------------
def event_of_length(n, emitter):
    """a Case B event (t1, t2 = FILTER) whose encoding is exactly n bytes"""
    ev = stamped(emitter, [entry("t1", T[0]), entry("t2", T[1]), entry("d", bytes(100))])
    d = n - (len(ev) - 100)
    for fix in (0, -1, -2, -3, 1, 2):  # (the data's own head changes width with its length)
        ev = stamped(emitter, [entry("t1", T[0]), entry("t2", T[1]), entry("d", data_bytes(d + fix, emitter & 0xFF))])
        if len(ev) == n:
            return ev
    raise AssertionError(n)


for _n in (65535, 65536, 65537):
    _e = event_of_length(_n, 6000)
    assert len(_e) == _n
    rcase(f"event_of_encoded_length_{_n}", _leaf(5, {3: _e, 4: SIB}), [(f"{t}", f, x) for t, f, x in perturbed(3, _e)] + [("sibling", at_index(4, SIB), 1)])
for _n in (0, 31, 32, 33, 65400):
    _e = stamped(6100, [entry("t1", T[0]), entry("t2", T[1]), entry("d", data_bytes(_n, 11))])
    rcase(f"data_of_{_n}_bytes", _leaf(5, {0: SIB, 7: _e}), perturbed(7, _e))
    if _n in (32, 33):
        _f = at_index(7, _e)
        _hexd = _f["data"]
        rcase(f"data_of_{_n}_bytes_wrong_in_byte_16", _leaf(5, {7: _e, 8: SIB}), [("byte_16", {**_f, "data": _hexd[:34] + flip_last(_hexd[34:36]) + _hexd[36:]}, 16),
                                                                                ("byte_15", {**_f, "data": _hexd[:32] + flip_last(_hexd[32:34]) + _hexd[34:]}, 16),
                                                                                ("byte_31", {**_f, "data": _hexd[:64] + flip_last(_hexd[64:66]) + _hexd[66:]}, 16)])
for _n in (0, 1, 2, 3, 4, 9, 255, 256):
    _e = stamped(6200 + _n, [entry("topics", b"".join(topic(k + 1) for k in range(_n))), entry("data", data_bytes(17, _n))])
    rcase(f"case_a_with_{_n}_topics", _leaf(5, {1: _e, 2: SIB}), perturbed(1, _e))
for _n in (1, 2, 3, 4):
    _e = good_event(6300 + _n, topics=tuple(range(_n)), n_data=20)
    _cl = perturbed(0, _e)
    if _n >= 3:  # the batched compare splits at two topics: a claim right in the first two and wrong in the last
        _f = at_index(0, _e)
        _cl.append(("first_byte_of_the_last_topic", {**_f, "topics": _f["topics"][:-1] + ["0x" + flip_last(_f["topics"][-1][2:4]) + _f["topics"][-1][4:]]}, 15))
        _cl.append(("wrong_in_the_third_topic_only", {**_f, "topics": _f["topics"][:2] + [hex0x(T[8])] + _f["topics"][3:]}, 15))
    rcase(f"case_b_with_{_n}_topics", _leaf(5, {0: _e}), _cl)

# --- every StampedEvent spelling of spelling_cases(), inside an events AMT, beside a well-formed sibling ---------------------------
for _k, (_name, _ev, _em, _bad) in enumerate(spelling_cases()):
    _j = (_k * 5) % 32
    _cl = [("not_a_log", {"event_index": _j, "emitter": _em, "topics": [], "data": "0x"}, 13),
           ("not_a_log_wrong_emitter", {"event_index": _j, "emitter": _em ^ 1, "topics": [], "data": "0x"}, 12)] if _bad else perturbed(_j, _ev)
    rcase("spelling " + _name, _leaf(5, {_j: _ev, (_j + 1) % 32: SIB}), _cl + [("sibling", at_index((_j + 1) % 32, SIB), 1)])

# --- decode errors the spellings do not have: the whole node fails, for the claimed index and for its sibling alike -----------------
_GOOD_ENTRIES = [entry("t1", T[0]), entry("t2", T[1])]
MALFORMED = {
    "entry_of_3_fields": stamped(7000, [array([uint(3), text("t1"), uint(0x55)])] + _GOOD_ENTRIES),
    "entry_of_5_fields": stamped(7001, _GOOD_ENTRIES + [array([uint(3), text("d"), uint(0x55), bstr(b"x"), NULL])]),
    "byte_string_key": stamped(7002, [array([uint(3), bstr(b"t1"), uint(0x55), bstr(T[0])])]),
    "text_value": stamped(7003, _GOOD_ENTRIES + [array([uint(3), text("d"), uint(0x55), text("data")])]),
    "negative_emitter": array([nint(-1), array(_GOOD_ENTRIES)]),
    "negative_flags": stamped(7004, [array([nint(-1), text("t1"), uint(0x55), bstr(T[0])])]),
    "indefinite_length_entries": array([uint(7005), b"\x9f" + b"".join(_GOOD_ENTRIES) + b"\xff"]),
    "indefinite_length_value": stamped(7006, [array([uint(3), text("t1"), uint(0x55), b"\x5f" + bstr(T[0]) + b"\xff"])]),
    "key_not_utf8": stamped(7007, [array([uint(3), head(3, 2) + b"\xc3\x28", uint(0x55), bstr(T[0])])]),
    "stamped_event_of_3_fields": array([uint(7008), array(_GOOD_ENTRIES), NULL]),
    "actor_event_is_a_map": array([uint(7009), cmap([("t1", bstr(T[0]))])]),
    "event_is_null": NULL,
}
for _name, _ev in MALFORMED.items():
    rcase(f"malformed_{_name}_at_the_claimed_index", _leaf(5, {2: _ev, 3: SIB}), [("claimed", {"event_index": 2, "emitter": 7000, "topics": [], "data": "0x"}, 66)])
    rcase(f"malformed_{_name}_at_a_sibling", _leaf(5, {3: SIB, 30: _ev}), [("sibling", at_index(3, SIB), 66), ("clear_bit", at_index(4, SIB), 66)])


def chunks(n: int) -> int:
    """128-byte lines a block of n bytes takes in the arena"""
    return max(1, (n + 127) // 128)


def _last_block_tipset():
    """An event that ends on the last byte of the LAST block of the arena.  The engine lays the arena out by 128-byte chunk
    count, most chunks first, and keeps the host table's order inside a class (csrc/host/witness.cpp, the K1 layout): the
    events root here is in the smallest class and the last entry of the store's table, so nothing but the arena's tail
    follows the event's last byte."""
    ev = stamped(5, [entry("t1", T[0])])
    msgs = [([M("x0"), M("x1")], [M("x2"), M("x3")])]
    st, claim, parts = tipset(msgs=msgs, receipts={0: lambda s: pyamt.receipt(events_root=events_root(s, {0: ev}, bw=1))}, at=(0, 0), event=ev, salt=77)
    root = next(c for c, b in st.blocks.items() if b.endswith(ev))
    st.blocks[root] = st.blocks.pop(root)  # the last entry of the (insertion-ordered) table
    assert list(st.blocks)[-1] == root and chunks(len(st.blocks[root])) == min(chunks(len(b)) for b in st.blocks.values()) == 1
    parts["events_root"] = root
    return st, claim, parts


_st, _claim, _parts = _last_block_tipset()
CASES["event_ends_on_the_last_byte_of_the_last_block_of_the_arena"] = (_st, _claim, 1)
META["event_ends_on_the_last_byte_of_the_last_block_of_the_arena"] = {"trust": None, "filter": None, "scan": None, "parts": _parts, "dropped": []}
_st, _claim, _parts = _last_block_tipset()
_claim["topics"] = [flip_last(_claim["topics"][0])]
CASES["event_ends_on_the_last_byte_of_the_last_block_of_the_arena_wrong_last_nibble"] = (_st, _claim, 15)
META["event_ends_on_the_last_byte_of_the_last_block_of_the_arena_wrong_last_nibble"] = {"trust": None, "filter": None, "scan": None, "parts": _parts, "dropped": []}


# --- every receipt case in a small tipset of its own -----------------------------------------------------------------------------------
def _wrap_receipt_cases():
    for name, make_root, claim_list in RC:
        for tag, fields, expect in claim_list:
            full = f"{name} / {tag}"
            assert full not in CASES, full
            salt = int.from_bytes(hashlib.sha256(name.encode()).digest()[:3], "big")
            st, claim, parts = tipset(salt=salt, msgs=[([A, B_], [C_])], at=(1, 0), event=SIB,
                                      receipts={0: lambda s: pyamt.receipt(), 1: lambda s: pyamt.receipt(events_root=make_root(s)), 2: lambda s: pyamt.receipt()})
            claim.update(fields)
            CASES[full] = (st, claim, expect)
            META[full] = {"trust": None, "filter": None, "scan": None, "parts": parts, "dropped": [], "rc": name}


_wrap_receipt_cases()


# ===== filter and trust over cases from above ==========================================================================================
def _matches(claim, filt):
    """does the CLAIMED log satisfy the filter — for a claim whose literal is 1 the claimed log is the event's"""
    t = claim["topics"]
    return len(t) >= 2 and t[0].lower() == hex0x(filt[0]) and t[1].lower() == hex0x(filt[1])


def under_filter(expect, claim, filt):
    """The literal of a claim under a filter, from its literal without one: 17 comes only after everything else
    (verifier.rs:247-251), so anything but 1 stays what it is, and a 1 becomes 17 exactly where the (verified, hence the
    claimed) log does not carry the filter's two topics."""
    return expect if expect != 1 else (1 if _matches(claim, filt) else 17)


def _filter_and_trust_variants():
    """The same claim under a filter: 17 comes only after everything else, so a literal other than 1 stays what it is and a 1
    becomes 17 exactly where the (verified) log does not carry the filter's two topics.  Under a trust policy: a claim
    whose strings parse answers the policy's status before any block is read; 69 from a parent or child string stays."""
    picked = [n for n in CASES if n.endswith("/ honest") or n.endswith("/ last_topic") or n.endswith("/ not_a_log")][::2][:40]
    picked += ["wrong_emitter", "no_event", "missing_events_root", "topic_count_one_less", "data_last_nibble", "not_an_evm_log"]
    for n in picked:
        st, claim, expect = CASES[n]
        for tag, filt in (("filter_0_1", FILTER), ("filter_0_2", OTHER_FILTER)):
            want = under_filter(expect, claim, filt)
            CASES[f"{n} / {tag}"] = (st, claim, want)
            META[f"{n} / {tag}"] = {**META[n], "filter": filt, "scan": None}
    step1 = {"claim_parent0_garbage": 69, "claim_child_garbage": 69}  # literals that stay: the strings are parsed before trust
    for n in ["base_true", "missing_child_header", "parents_mismatch_order", "claim_message_garbage", "wrong_emitter", "txmeta_as_a_3_tuple",
              "spelling B 2 topics / honest", "malformed_text_value_at_a_sibling / sibling", "claim_parent0_garbage", "claim_child_garbage"]:
        st, claim, expect = CASES[n]
        for tag, (policy, status) in TRUST.items():
            want = step1.get(n, expect if status is None else status)
            CASES[f"{n} / trust_{tag}"] = (st, claim, want)
            META[f"{n} / trust_{tag}"] = {**META[n], "trust": policy, "scan": None}


_filter_and_trust_variants()


# ===== one tipset whose receipts carry every receipt case =============================================================================
_ONE = None


def one_tipset():
    """→ (store, parts, names, claims, expected): receipt i is receipt case i (the messages split over the four message AMTs
    of two parent blocks, two of them repeated in the second), and
    every claim of every receipt case, in receipt order"""
    global _ONE
    if _ONE is None:
        n = len(RC)
        m = [M(f"one{i}") for i in range(n)]
        msgs = [(m[: n // 3], m[n // 3: n // 2]), (m[n // 2: n - 5] + m[:2], m[n - 5:])]
        receipts = {i: (lambda mk: lambda s: pyamt.receipt(events_root=mk(s)))(mk) for i, (_n, mk, _c) in enumerate(RC)}
        st, base, parts = tipset(msgs=msgs, receipts=receipts, at=(0, 0), event=SIB, salt=4242)
        names, cl, want = [], [], []
        for i, (name, _mk, claim_list) in enumerate(RC):
            for tag, fields, expect in claim_list:
                names.append(f"{name} / {tag}")
                cl.append({**base, "exec_index": i, "message_cid": cid_str(m[i]), **fields})
                want.append(expect)
        _ONE = (st, parts, names, cl, want)
    return _ONE


def second_tipset():
    """another small pair (other epochs, other messages) to merge with the default one: two contexts in one witness"""
    m = [M(f"second{i}") for i in range(5)]
    return tipset(msgs=[(m[:2], m[2:3]), (m[3:], [])], at=(4, 0), parent_epoch=PARENT_EPOCH + 10, child_epoch=CHILD_EPOCH + 10, salt=999)


# ---- helpers the two test files share ----------------------------------------------------------------------------------------------------
def proofs(claim_list):
    """claim dicts → an object with .arr (ctypes ipcfp_event_proof_t[n]) and .n, owning the strings"""
    import bundle_ref

    return bundle_ref.claims_from_parsed({"event_proofs": claim_list, "storage_proofs": []})[0]


def trust_policy(t):
    return None if t is None else claims_mod.TrustPolicy(kind=1, ec_chain_empty=t[0], min_epoch=t[1], max_epoch=t[2])


def event_filter(f):
    return None if f is None else claims_mod.make_filter(f[0], f[1])


# ---- the structured mutator --------------------------------------------------------------------------------------------------------------
CLAIM_EDITS = (
    lambda c, rng: {"event_index": (0, 1, 2, 3, 31, 32, 1 << 32, (1 << 64) - 1)[int(rng.integers(8))]},
    lambda c, rng: {"exec_index": int(rng.integers(0, 8))},
    lambda c, rng: {"emitter": c["emitter"] + int(rng.integers(1, 3))},
    lambda c, rng: {"topics": c["topics"][:-1]},
    lambda c, rng: {"topics": c["topics"][:-1] + [flip_last(c["topics"][-1])]} if c["topics"] else {"topics": [hex0x(T[0])]},
    lambda c, rng: {"data": c["data"] + "00"},
    lambda c, rng: {"data": flip_last(c["data"])} if len(c["data"]) > 2 else {"data": "0x00"},
    lambda c, rng: {"message_cid": cid_str(M(int(rng.integers(0, 7))))},
    lambda c, rng: {"message_cid": c["message_cid"][:-3]},
    lambda c, rng: {"child_epoch": c["child_epoch"] + 1},
    lambda c, rng: {"parent_epoch": c["parent_epoch"] - 1},
    lambda c, rng: {"parent_tipset_cids": c["parent_tipset_cids"][::-1]},
    lambda c, rng: {"child_block_cid": c["parent_tipset_cids"][0]},
)


def mutated_tipset(rng):
    """The default tipset with a random honest claim and ONE thing changed: a field of one block re-spelled (wrong major type,
    length ± 1, null, non-minimal head, swapped link — nothing above it is re-hashed: the store keeps the new bytes under
    the old CID), a block dropped, or a claim field edited; sometimes a filter or a trust window on top.  Blocks on the
    receipt side of the chain (the receipts tree, events roots) are picked twice as often as the headers and message
    AMTs in front of them, so that the later steps of the verifier get their share.
    → (blocks dict, claim, trust, filter)"""
    e = int(rng.choice([0, 2, 2, 2, 3, 4, 5]))
    j = int(rng.integers(0, 3)) if e == 2 else 0
    st, claim, parts = tipset(salt=int(rng.integers(1 << 20)), at=(e, j))
    blocks = st.blocks
    front = set(parts["parents"]) | set(parts["txmeta"]) | {parts["child"]} | {parts[f"{w}{k}"] for w in ("bls", "secp") for k in (0, 1)}
    back = [c for c in blocks if c not in front]
    kind = int(rng.integers(10))
    if kind < 5:
        pool = back if rng.integers(3) else sorted(front)
        c = pool[int(rng.integers(len(pool)))]
        if rng.integers(8) == 0:
            del blocks[c]
        else:
            blocks[c] = encode(mutate_field(pystorage.decode(blocks[c]), rng, list(blocks)))
    elif kind < 9:
        claim.update(CLAIM_EDITS[int(rng.integers(len(CLAIM_EDITS)))](claim, rng))
    trust = filt = None
    if rng.integers(8) == 0:
        trust = (0, PARENT_EPOCH - int(rng.integers(0, 2)), CHILD_EPOCH + 1) if rng.integers(3) else (0, CHILD_EPOCH, CHILD_EPOCH + 9)
    if rng.integers(4) == 0:
        filt = FILTER if rng.integers(2) else OTHER_FILTER
    return blocks, claim, trust, filt
