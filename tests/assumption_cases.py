"""The ⚠ ASSUMPTIONS about the un-vendored crates (serde_ipld_dagcbor 0.6, cid 0.10/0.11, fvm_ipld_amt 0.7.4,
fvm_shared 4.7 — Cargo.toml:11-22, no lockfile, no tests in the reference), one hand-written block per assumption.

Neither the oracle nor the engine can be checked against the crates here (no Rust toolchain, no vendored sources): these
cases state, by NAME, what both were written to do, so that the day a real-chain fixture or the crate sources are at
hand each assumption is confirmed or flipped in ONE place — tests/test_assumptions.py runs the table against the
oracle (CPU) and against the engine (GPU) and both must give the status listed here.

Each case: name → (blocks, root cid, AMT version, value kind, index, expected status); statuses as in include/ipcfp.h
(1 = found, 32 = NOT_FOUND, 66 = ERR_DECODE).  The carrier is always a one-level Amt (v3) whose single value, or whose
own header, carries the spelling in question."""
import pyamt
from pyamt import array, bstr, head, link, uint

TRUE, NOT_FOUND, ERR_DECODE = 1, 32, 66


def _leaf_root(value: bytes, bitmap: int = 0x01, count: bytes = None, values_header: bytes = None, trailer: bytes = b""):
    """v3 root [bit_width 3, height 0, count, [bitmap, [], [value]]] as raw bytes"""
    vals = (values_header if values_header is not None else head(4, 1)) + value
    node = head(4, 3) + bstr(bytes([bitmap])) + head(4, 0) + vals
    return head(4, 4) + uint(3) + uint(0) + (count if count is not None else uint(1)) + node + trailer


def _case(block: bytes, kind: str, index: int, expect: int):
    s = pyamt.Store()
    root = s.put(block)
    return s, root, 3, kind, index, expect


CID = pyamt.cid_of(b"\x80")
CASES = {
    # --- serde_ipld_dagcbor: what a strict DAG-CBOR decode accepts -------------------------------------------------
    "baseline_minimal_encoding_is_found": lambda: _case(_leaf_root(uint(7)), "any", 0, TRUE),
    "nonminimal_uint_argument_is_accepted": lambda: _case(_leaf_root(uint(7), count=b"\x18\x01"), "any", 0, TRUE),
    "nonminimal_array_length_is_accepted": lambda: _case(_leaf_root(uint(7), values_header=b"\x98\x01"), "any", 0, TRUE),
    "indefinite_length_array_is_rejected": lambda: _case(_leaf_root(uint(7) + b"\xff", values_header=b"\x9f"), "any", 0, ERR_DECODE),
    "float64_is_accepted": lambda: _case(_leaf_root(b"\xfb" + bytes(8)), "any", 0, TRUE),
    "float32_is_rejected": lambda: _case(_leaf_root(b"\xfa" + bytes(4)), "any", 0, ERR_DECODE),
    "float16_is_rejected": lambda: _case(_leaf_root(b"\xf9" + bytes(2)), "any", 0, ERR_DECODE),
    "undefined_simple_value_is_rejected": lambda: _case(_leaf_root(b"\xf7"), "any", 0, ERR_DECODE),
    "only_tag_42_is_a_legal_tag": lambda: _case(_leaf_root(b"\xc1" + uint(5)), "any", 0, ERR_DECODE),
    "text_must_be_utf8": lambda: _case(_leaf_root(head(3, 2) + b"\xc3\x28"), "any", 0, ERR_DECODE),
    "trailing_bytes_after_the_block_item_are_rejected": lambda: _case(_leaf_root(uint(7), trailer=b"\x00"), "any", 0, ERR_DECODE),
    # --- cid: the bytes of a link ---------------------------------------------------------------------------------------
    "link_is_tag42_bytes_with_identity_prefix": lambda: _case(_leaf_root(link(CID)), "cid", 0, TRUE),
    "link_without_the_00_multibase_prefix_is_rejected": lambda: _case(_leaf_root(b"\xd8\x2a" + bstr(CID)), "cid", 0, ERR_DECODE),
    "cid_with_bytes_after_the_digest_is_rejected": lambda: _case(_leaf_root(b"\xd8\x2a" + bstr(b"\x00" + CID + b"\x00")), "cid", 0, ERR_DECODE),
    "cid_with_nonminimal_varint_is_rejected": lambda: _case(_leaf_root(b"\xd8\x2a" + bstr(b"\x00\x81\x00" + CID[1:])), "cid", 0, ERR_DECODE),
    # --- fvm_ipld_amt: the node --------------------------------------------------------------------------------------------
    "amt_bitmap_is_lsb_first_bit1_is_index1": lambda: _case(_leaf_root(uint(7), bitmap=0x02), "any", 1, TRUE),
    "amt_bitmap_is_lsb_first_bit1_is_not_index6": lambda: _case(_leaf_root(uint(7), bitmap=0x02), "any", 6, NOT_FOUND),
    "amt_value_count_must_match_the_bitmap": lambda: _case(_leaf_root(uint(7), bitmap=0x03), "any", 0, ERR_DECODE),
    "amt_count_field_is_not_checked_by_load_or_get": lambda: _case(_leaf_root(uint(7), count=uint(9)), "any", 0, TRUE),
    # --- fvm_shared / serde: typed values ----------------------------------------------------------------------------------
    "vec_u8_is_an_array_of_small_uints": lambda: _case(_leaf_root(array([uint(1), uint(255)])), "vec_u8", 0, TRUE),
    "vec_u8_is_not_a_byte_string": lambda: _case(_leaf_root(bstr(b"\x01\x02")), "vec_u8", 0, ERR_DECODE),
    "vec_u8_element_above_255_is_rejected": lambda: _case(_leaf_root(array([uint(256)])), "vec_u8", 0, ERR_DECODE),
    "receipt_is_a_4_tuple_with_nullable_events_root": lambda: _case(_leaf_root(pyamt.receipt()), "receipt", 0, TRUE),
    "receipt_with_a_fifth_field_is_rejected": lambda: _case(_leaf_root(head(4, 5) + uint(0) + bstr(b"") + uint(1) + b"\xf6" + uint(0)), "receipt", 0, ERR_DECODE),
    "receipt_exit_code_above_u32_is_rejected": lambda: _case(_leaf_root(head(4, 4) + uint(1 << 32) + bstr(b"") + uint(1) + b"\xf6"), "receipt", 0, ERR_DECODE),
}


# --- serde's derive and fvm_ipld_hamt, carried by a storage chain (tests/storage_chain_cases.py `chain`) -------------------
# Each case: name → callable → (store, claim fields, expected status of verify_storage_proof).  tests/pystorage.py names each
# assumption with a constant and makes the SAME choice the oracle and the engine were written to make: on these points the
# three are one judge, and a case here pins what they do, it does not prove the crate does it.  tests/test_storage_chain.py
# holds pystorage and the oracle to the table, tests/test_gpu_storage_chain.py every route of the engine;
# tests/storage_chain_cases.py takes the cases into its own table, so they also run merged into one witness.
def _sc():
    import storage_chain_cases as sc

    return sc


def _storage_case(root_block, slot: bytes, value: bytes, expect: int, parts=False):
    """root_block: the contract-state root's bytes, or callable(store) → bytes"""
    import hashlib

    salt = int.from_bytes(hashlib.sha256(slot + value + bytes([expect])).digest()[:3], "big")
    store, claim, made = _sc().chain(root_block if callable(root_block) else (lambda st: root_block), slot, value, salt=salt)
    return (store, claim, expect, made["dropped"]) if parts else (store, claim, expect)


def _bucket_node(keys_and_bytes):
    """a width-5 root node with ONE bucket at index 17 holding the pairs as given (value: Vec<u8>)"""
    sc = _sc()
    return sc.node(1 << 17, [sc.bucket([(k, sc.vec(v)) for k, v in keys_and_bytes])])


def _keys_at_17(n):
    sc = _sc()
    return sorted(sc.slot_with_index(17, k) for k in range(n))


def _b1_saying(width_said):
    """B1 `[root, bitwidth]` over a tree built at width 5"""
    sc = _sc()
    return lambda st: array([link(sc.pyhamt.build_hamt(st, sc.hamt_items(sc.MANY), 5)), uint(width_said)])


_SLOT, _VALUE = bytes(range(32)), b"\x2a"
_PAIRS = array([array([bstr(_SLOT), bstr(_VALUE)])])
_B01 = array([bstr(b"\x01"), array([])])  # `[h'01', []]`
STORAGE_CASES = {
    # STRUCT_FROM_ARRAY_IS_REJECTED.  A serde-derived struct (`SmallMap`, `MapStruct`: storage/decode.rs:10-13,28-32) is read
    # from a CBOR MAP only.  Its fields offered as an ARRAY `[v]` — serde's derive has a visit_seq that would take them — are a
    # decode error of that attempt: pystorage, the oracle and the engine all refuse it, and nothing later fits an array of 1
    # (at C it is no HAMT node), so the call is ERR_DECODE where an accepting decoder would answer TRUE.
    "struct_offered_as_an_array_is_rejected": lambda **o: _storage_case(array([_PAIRS]), _SLOT, _VALUE, ERR_DECODE, **o),
    "the_same_struct_as_a_map_is_found": lambda **o: _storage_case(head(5, 1) + head(3, 1) + b"v" + _PAIRS, _SLOT, _VALUE, TRUE, **o),
    # … and inside A2: `[params, [v]]` is then an A1 whose list holds a non-map — no attempt takes it; at C the one "pointer" is
    # a bucket whose value is a byte string, no Vec<u8>
    "struct_offered_as_an_array_inside_a2_is_rejected": lambda **o: _storage_case(array([bstr(b""), array([_PAIRS])]), _SLOT, _VALUE, ERR_DECODE, **o),
    # HAMT_POINTER_COUNT_IS_CHECKED_WHEN_INDEXED.  `[h'01', []]` decodes as an A1 with an empty list, falls through
    # (storage/decode.rs:47) and is, at C, a node whose bitfield names a pointer it does not have.  All three compare
    # popcount and pointer list only where a get indexes the list: an Err for a key that lands on bit 0, a clear bit — zero,
    # TRUE — for any other key.  A crate that compares them when it DECODES the node gives ERR_DECODE for both, as
    # the AMT does (amt_value_count_must_match_the_bitmap above); flip the second case then.
    "a1_bitfield_01_empty_list_key_on_bit_0": lambda **o: _storage_case(_B01, _sc().slot_with_index(0), b"", ERR_DECODE, **o),
    "a1_bitfield_01_empty_list_key_on_bit_9": lambda **o: _storage_case(_B01, _sc().slot_with_index(9), b"", TRUE, **o),
    # HAMT_BUCKET_SIZE_AND_ORDER_ARE_NOT_CHECKED_ON_READ.  SURVEY.md A.6 gives the bucket as "≤ 3, sorted by key" — what a
    # writer produces — and the get as a linear search.  All three search the bucket as it stands; a crate that enforces either
    # property on read gives ERR_DECODE for these two.
    "c_bucket_of_4_fourth_key": lambda **o: _storage_case(_bucket_node([(k, bytes([i + 1])) for i, k in enumerate(_keys_at_17(4))]),
                                                          _keys_at_17(4)[3], b"\x04", TRUE, **o),
    "c_bucket_unsorted": lambda **o: _storage_case(_bucket_node([(_keys_at_17(3)[i], bytes([i + 1])) for i in (2, 0, 1)]),
                                                   _keys_at_17(3)[0], b"\x01", TRUE, **o),
    # HAMT_BIT_WIDTH_OUTSIDE_1_TO_8_IS_AN_ERR_OF_THE_GET.  `load_with_bit_width` takes any u32; all three report a width of 0 or
    # of more than 8 as ERR_DECODE — the Err of `HashBits::next` — once the root is loaded.  (That the root is FETCHED first
    # is the reference's text, storage/decode.rs:79-80, and no assumption: storage_chain_cases b1_bit_width_0_and_inner_root_absent.)
    "b1_bit_width_0": lambda **o: _storage_case(_b1_saying(0), _sc().S[0], _sc().VAL[0], ERR_DECODE, **o),
    "b1_bit_width_9": lambda **o: _storage_case(_b1_saying(9), _sc().S[0], _sc().VAL[0], ERR_DECODE, **o),
}


# --- the same assumptions as the GET PRIMITIVES meet them (tests/hamt_get_cases.py) -----------------------------------------
# Each case: name → callable(value kind) → (store, root CID, bit width, [(key, expected status, value bytes | None)], the
# limit it stands at | None), or None where the kind has no such case.  tests/hamt_get_cases.py takes them into its table:
# tests/test_hamt_get_cases.py holds pystorage and the oracle to them, tests/test_gpu_hamt_get_cases.py every route.
def _hg():
    import hamt_get_cases as hg

    return hg


def _get_case(node_of, probes_of, bw=5, limit=None):
    """node_of(hg, kind) → the root node's bytes; probes_of(hg, kind) → [(key, status, value)]"""
    def make(kind):
        hg = _hg()
        st = pyamt.Store()
        return st, st.put(node_of(hg, kind)), bw, probes_of(hg, kind), limit
    return make


def _one_bucket(hg, kind, n, j=17, order=None):
    keys = sorted(hg.K((), j, k) for k in range(n))
    if order is not None:
        keys = [keys[i] for i in order]
    return keys, hg.build_node({j: hg.bucket([(k, hg.val(kind, k)) for k in keys])})


def _big_bucket(n):
    def probes(hg, kind):
        keys, _ = _one_bucket(hg, kind, n)
        return [(keys[0], TRUE, hg.val(kind, keys[0])), (keys[-1], TRUE, hg.val(kind, keys[-1])),
                (keys[n // 2], TRUE, hg.val(kind, keys[n // 2])), (hg.K((), 17, n), NOT_FOUND, None)]
    return _get_case(lambda hg, kind: _one_bucket(hg, kind, n)[1], probes, limit=("bucket", n))


def _node_of_97(hg, kind):
    """31 buckets of 3 and one of 4 on child indices 0 … 31: 97 pairs"""
    at, pairs = {}, []
    for j in range(32):
        keys = sorted(hg.K((), j, k) for k in range(4 if j == 31 else 3))
        at[j] = hg.bucket([(k, hg.val(kind, k)) for k in keys])
        pairs += keys
    return hg.build_node(at), pairs


def _respelled_key(spell):
    """a node whose one bucket holds [key, value] with the KEY's head spelled by `spell(len)`; the key is found by its bytes"""
    def node_of(hg, kind):
        k = hg.K((), 17)
        return hg.build_node({17: array([array([spell(len(k)) + k, hg.val(kind, k)])])})
    return _get_case(node_of, lambda hg, kind: [(hg.K((), 17), TRUE, hg.val(kind, hg.K((), 17))), (hg.K((), 17, 1), NOT_FOUND, None)])


def _respelled_actor(field):
    def make(kind):
        if kind == "vec_u8":
            return None
        hg = _hg()
        i = hg.vi(hg.K((), 17))
        v = hg.astate(i, seq=b"\x18\x05") if field == "sequence" else hg.astate(i, adr=b"\x58\x15\x01" + bytes(range(20)))
        st = pyamt.Store()
        return st, st.put(hg.build_node({17: hg.bucket([(hg.K((), 17), v)])})), 5, [(hg.K((), 17), TRUE, v)], None
    return make


def _width_out_of_range(bw):
    def make(kind):
        hg = _hg()
        keys, items = hg.width_items(kind)
        st = pyamt.Store()
        root = hg.pyhamt.build_hamt(st, items, 5)
        return st, root, bw, [(keys[0], ERR_DECODE, None), (b"no such key", ERR_DECODE, None)], ("width", bw)
    return make


def _counts(bits, n_pointers):
    """a width-5 node whose bitfield has `bits` set over n_pointers one-pair buckets (for the lowest set bits, in order)"""
    def node_of(hg, kind):
        ptrs = [hg.bucket([(hg.K((), j), hg.val(kind, hg.K((), j)))]) for j in (list(bits) + [30, 31])[:n_pointers]]
        return hg.node(sum(1 << j for j in bits), ptrs)
    return node_of


HAMT_GET_CASES = {
    # HAMT_POINTER_COUNT_IS_CHECKED_WHEN_INDEXED: an Err only for the key that lands on the pointer that is not there
    "popcount_above_the_pointer_count": _get_case(_counts((2, 9, 20), 2), lambda hg, kind: [
        (hg.K((), 2), TRUE, hg.val(kind, hg.K((), 2))), (hg.K((), 9), TRUE, hg.val(kind, hg.K((), 9))),
        (hg.K((), 20), ERR_DECODE, None), (hg.K((), 5), NOT_FOUND, None)]),
    "popcount_below_the_pointer_count": _get_case(_counts((2, 9), 3), lambda hg, kind: [
        (hg.K((), 2), TRUE, hg.val(kind, hg.K((), 2))), (hg.K((), 9), TRUE, hg.val(kind, hg.K((), 9))),
        (hg.K((), 30), NOT_FOUND, None), (hg.K((), 5), NOT_FOUND, None)]),
    "empty_bitfield_over_a_pointer": _get_case(_counts((), 1), lambda hg, kind: [(hg.K((), 30), NOT_FOUND, None), (hg.K((), 0), NOT_FOUND, None)]),
    # HAMT_BUCKET_SIZE_AND_ORDER_ARE_NOT_CHECKED_ON_READ: the bucket is searched as it stands, the first match wins
    "node_of_97_entries": _get_case(lambda hg, kind: _node_of_97(hg, kind)[0], lambda hg, kind: [
        (_node_of_97(hg, kind)[1][0], TRUE, hg.val(kind, _node_of_97(hg, kind)[1][0])),
        (_node_of_97(hg, kind)[1][-1], TRUE, hg.val(kind, _node_of_97(hg, kind)[1][-1])),
        (hg.K((), 31, 4), NOT_FOUND, None)], limit=("entries", 97)),
    "one_bucket_of_97_entries": _big_bucket(97),
    "one_bucket_of_256_entries": _big_bucket(256),
    "empty_bucket": _get_case(lambda hg, kind: hg.build_node({17: array([])}), lambda hg, kind: [(hg.K((), 17), NOT_FOUND, None), (hg.K((), 3), NOT_FOUND, None)]),
    "unsorted_bucket": _get_case(lambda hg, kind: _one_bucket(hg, kind, 3, order=(2, 0, 1))[1],
                                 lambda hg, kind: [(k, TRUE, hg.val(kind, k)) for k in _one_bucket(hg, kind, 3)[0]] + [(hg.K((), 17, 3), NOT_FOUND, None)]),
    "same_key_twice_the_first_wins": _get_case(
        lambda hg, kind: hg.build_node({17: hg.bucket([(hg.K((), 17), hg.val(kind, b"first")), (hg.K((), 17), hg.val(kind, b"second"))])}),
        lambda hg, kind: [(hg.K((), 17), TRUE, hg.val(kind, b"first"))]),
    # HAMT_BIT_WIDTH_OUTSIDE_1_TO_8_IS_AN_ERR_OF_THE_GET, on a root that exists (a missing root is 65 by the reference's own
    # text: tests/hamt_get_cases.py width_*_root_missing)
    **{f"width_{bw}_on_a_root_that_exists": _width_out_of_range(bw) for bw in (0, 9, 32, (1 << 32) - 1)},
    # a non-minimal head is accepted (nonminimal_uint_argument_is_accepted above), also where a fast parse expects the short one
    "key_head_58_nn_below_24": _respelled_key(lambda n: bytes([0x58, n])),
    "key_head_59_00_nn": _respelled_key(lambda n: bytes([0x59, 0, n])),
    "actor_state_sequence_spelled_18_05": _respelled_actor("sequence"),
    "actor_state_address_header_58_15": _respelled_actor("address"),
}


# --- fvm_ipld_amt and fvm_shared as the EVENT chain meets them (tests/event_chain_cases.py `tipset`) ----------------------------
# Each case: name → callable → (store, claim fields, expected status of verify_event_proof).  tests/pyevents.py names each
# assumption with a constant and makes the choice the oracle and the engine were written to make; a case here pins what the
# three do, it does not prove the crate does it.  tests/test_event_chain.py holds pyevents and the oracle to the table,
# tests/test_gpu_event_chain.py every route of the engine.
def _ec():
    import event_chain_cases as ec

    return ec


def _event_case(make_root, fields: dict, expect: int, salt: int):
    """receipt 2 of the default tipset gets the events root `make_root(store)`; the claim names it with `fields`"""
    ec = _ec()
    store, claim, _ = ec.tipset(salt=salt, receipts={**ec.default_receipts(6), 2: lambda st: pyamt.receipt(events_root=make_root(st))})
    claim.update(fields)
    return store, claim, expect


def _ev(emitter=900):
    return _ec().good_event(emitter)


def _claim_for(j, emitter=900, **over):
    return {"event_index": j, **_ec().log_fields(_ev(emitter)), **over}


def _root(bw=5, height=0, count=1, bitmap=b"\x01\x00\x00\x00", values=None, links=()):
    ec = _ec()
    return lambda st: ec.raw_root(st, [_ev()] if values is None else values, bitmap, bw=bw, height=height, count=uint(count), links=links)


def _entry_event(flags, codec):
    ec = _ec()
    return ec.stamped(900, [ec.entry("t1", ec.T[0], flags=flags, codec=codec), ec.entry("t2", ec.T[1], flags=flags, codec=codec)])


EVENT_CASES = {
    # AMT_COUNT_IS_NOT_CHECKED
    "events_root_count_0_over_one_value": lambda: _event_case(_root(count=0), _claim_for(0), TRUE, 1),
    "events_root_count_2_pow_40_over_one_value": lambda: _event_case(_root(count=1 << 40), _claim_for(0), TRUE, 2),
    # AMT_MAX_HEIGHT_IS_64_OVER_BIT_WIDTH: at bit width 8 a height of 8 loads, 9 is an Err of the load
    "events_root_height_8_at_bit_width_8_loads": lambda: _event_case(_root(bw=8, height=8, count=0, bitmap=bytes(32), values=[]), _claim_for(0), 11, 3),
    "events_root_height_9_at_bit_width_8": lambda: _event_case(_root(bw=8, height=9, count=0, bitmap=bytes(32), values=[]), _claim_for(0), ERR_DECODE, 4),
    "events_root_height_13_at_bit_width_5": lambda: _event_case(_root(height=13, count=0, bitmap=bytes(4), values=[]), _claim_for(0), ERR_DECODE, 5),
    # … and at bit width 3, the width of every Amtv0 the enumerator walks (tests/amt_enum_cases.py "height_21_…", "height_22_…"):
    # 64 / 3 = 21 loads, 22 is an Err of the load
    "events_root_height_21_at_bit_width_3_loads": lambda: _event_case(_root(bw=3, height=21, count=0, bitmap=bytes(1), values=[]), _claim_for(0), 11, 15),
    "events_root_height_22_at_bit_width_3": lambda: _event_case(_root(bw=3, height=22, count=0, bitmap=bytes(1), values=[]), _claim_for(0), ERR_DECODE, 16),
    # AMT_MAX_INDEX_IS_U64_MAX_MINUS_1: the generic Err (64) for u64::MAX, None for the index below it
    "event_index_u64_max": lambda: _event_case(_root(), _claim_for((1 << 64) - 1), 64, 6),
    "event_index_u64_max_minus_1": lambda: _event_case(_root(), _claim_for((1 << 64) - 2), 11, 7),
    # AMT_LINKS_AT_HEIGHT_0_ARE_AN_ERR_OF_THE_WALK
    "events_root_height_0_with_a_link_index_0": lambda: _event_case(_root(values=[], links=[pyamt.cid_of(b"nowhere")]), _claim_for(0), ERR_DECODE, 8),
    "events_root_height_0_with_a_link_index_32": lambda: _event_case(_root(values=[], links=[pyamt.cid_of(b"nowhere")]), _claim_for(32), 11, 9),
    # AMT_BIT_WIDTH_IS_1_TO_8
    "events_root_bit_width_0": lambda: _event_case(_root(bw=0, bitmap=b"\x01"), _claim_for(0), ERR_DECODE, 10),
    "events_root_bit_width_9": lambda: _event_case(_root(bw=9, bitmap=b"\x01" + bytes(63)), _claim_for(0), ERR_DECODE, 11),
    # ENTRY_FLAGS_AND_CODEC_ARE_ANY_U64
    "entry_flags_and_codec_u64_max": lambda: _event_case(_root(values=[_entry_event((1 << 64) - 1, (1 << 64) - 1)]),
                                                          {"event_index": 0, **_ec().log_fields(_entry_event(0, 0))}, TRUE, 12),
    # serde_ipld_dagcbor accepts a non-minimal integer (nonminimal_uint_argument_is_accepted above), also where the event
    # table's fast decodes expect the short spelling: the emitter and a key's length
    "emitter_900_spelled_in_four_bytes": lambda: _event_case(_root(values=[b"\x82\x1a\x00\x00\x03\x84" + _ev()[4:]]), _claim_for(0), TRUE, 13),
    "emitter_5_spelled_in_two_bytes": lambda: _event_case(_root(values=[b"\x82\x19\x00\x05" + _ev()[4:]]), {**_claim_for(0), "emitter": 5}, TRUE, 14),
}
