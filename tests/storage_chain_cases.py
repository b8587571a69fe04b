"""Hand-built witnesses for `verify_storage_proof` (src/proofs/storage/verifier.rs:24-63), one NAMED case per spelling the
synthetic tipset writer never emits: name → (store, claim, expected status).  The expected status is a LITERAL written
down from the reference's Rust; tests/pystorage.py (an independent restatement) must reproduce every literal, and the
oracle (CPU) and every route of the engine (GPU) must give it too — tests/test_storage_chain.py,
tests/test_gpu_storage_chain.py.

`chain()` writes a minimal valid chain with pyamt's encoders and pyhamt: child header → StateRoot → actors HAMT (a
handful of actors) → ActorState → EvmState → contract-state root, and returns (store, claim fields, parts).  A case
breaks it in ONE place unless its group says otherwise: a block is re-spelled BEFORE it is hashed (so the chain above
links to the defective block), or dropped from the store, or a claim string is edited.

Statuses as in include/ipcfp.h: 1 TRUE · 3 untrusted child · 18 state root ≠ · 19 actor state ≠ · 20 storage root ≠ ·
21 value ≠ · 65 block missing · 66 decode · 68 actor not found · 69 unparsable claim string · 70 HAMT max depth."""
import hashlib

import pyamt
import pyhamt
import pystorage
from pyamt import NULL, array, bstr, head, link, uint

LAYOUTS = ("A1", "A2", "A3", "B1", "B2", "C")
EPOCH = 1000
TRUST_WINDOW = (0, 900, 1100)  # (ec_chain_empty, min_epoch, max_epoch): the policy of the cases that carry one


# ---- encoders the two writers do not have --------------------------------------------------------------------------
def text(s):
    return head(3, len(s.encode())) + s.encode()


def cmap(pairs):
    """[(field name, encoded value)] → a CBOR map, entries in the order given (duplicates included)"""
    return head(5, len(pairs)) + b"".join(text(k) + v for k, v in pairs)


def nint(n):
    return head(1, -1 - n)


def vec(b):
    """serde Vec<u8>: an array of minimally encoded uints"""
    return array([uint(x) for x in b])


def slot(tag) -> bytes:
    return hashlib.sha256(b"slot:" + str(tag).encode()).digest()


def slot_with_index(idx, k=0, bw=5) -> bytes:
    """the k-th slot whose HAMT child index at depth 0 is `idx`"""
    i = 0
    while True:
        s = slot(f"idx{i}")
        if pyhamt.index_at(s, 0, bw) == idx:
            if k == 0:
                return s
            k -= 1
        i += 1


def node(bitfield: int, pointers) -> bytes:
    return array([bstr(bitfield.to_bytes((bitfield.bit_length() + 7) // 8, "big")), array(pointers)])


def bucket(pairs) -> bytes:
    return array([array([bstr(k), v]) for k, v in pairs])


def smap(pairs, before=(), after=()):
    """SmallMap { v: [[key, value]…] } with optional unknown fields around "v" """
    return cmap(list(before) + [("v", array([array([bstr(k), bstr(v)]) for k, v in pairs]))] + list(after))


def pad32(v: bytes) -> bytes:
    return v[-32:] if len(v) >= 32 else bytes(32 - len(v)) + v


def hex0x(b: bytes) -> str:
    return "0x" + b.hex()


def cid_str(cid: bytes) -> str:
    return pystorage.cid_to_string(cid)


OTHER = pyamt.cid_of(b"some other block")  # a well-formed CID of a block no witness holds


# ---- the chain ---------------------------------------------------------------------------------------------------------
def actor_key(n: int) -> bytes:
    out = bytearray(b"\0")
    while True:
        out.append((n & 0x7F) | (0x80 if n >> 7 else 0))
        n >>= 7
        if not n:
            return bytes(out)


def chain(root_block, slot32, value, *, salt=0, actor_id=1001, n_actors=6, header=None, state_root=None, actor=None,
          evm=None, drop=(), edit=None, root_sha256=False, root_last=False):
    """A valid chain around one contract-state root.
    root_block   callable(store) → the root block's bytes, or (bytes, [CIDs it removed from the store again]); it may put
                 inner blocks first
    slot32/value the claimed slot and the bytes the claim's value is the left_pad_32 of
    header, state_root, actor, evm   callable(default encoded fields) → the block's (value's) bytes, to re-spell it
    drop         names of parts ("child", "state_root", "actors", "actor_state", "root") or CIDs removed afterwards
    edit         claim fields overwritten at the end: a dict, or callable(finished claim, store) → dict
    root_sha256  the root block goes under a CIDv1 dag-cbor sha2-256 CID
    root_last    the root block is the LAST entry of the store's table — this orders the HOST table only: the engine lays
                 the arena out by its own schedule (longest blocks first, each on a 128-byte line)
    → (store, claim, parts)"""
    st = pyamt.Store()
    made = root_block(st)
    root_bytes, dropped = made if type(made) is tuple else (made, [])
    root = st.put(root_bytes, sha256_cid=root_sha256)
    code, bytecode, info, receipts, messages = (pyamt.cid_of(n.encode()) for n in ("code", "bytecode", "info", "rcpt", "msgs"))
    evm_fields = [link(bytecode), bstr(hashlib.sha256(b"bytecode").digest()), link(root), NULL, uint(1 + salt % 1000), NULL]
    astate = st.put(evm(evm_fields) if evm else array(evm_fields))
    actors = {}
    for k in range(n_actors):
        aid = actor_id + k
        state = astate if k == 0 else pyamt.cid_of(b"state of %d" % aid)
        fields = [link(code), link(state), uint(salt % 997), bstr(b"\x00\x05"), NULL]
        actors[actor_key(aid)] = actor(fields) if (actor and k == 0) else array(fields)
    actors_root = pyhamt.build_hamt(st, actors)
    sr_fields = [uint(5), link(actors_root), link(info)]
    sroot = st.put(state_root(sr_fields) if state_root else array(sr_fields))
    parent = pyamt.cid_of(b"parent header")
    hdr_fields = [bstr(b"\x00\xe8\x07"), array([bstr(b"vrf")]), NULL, array([]), array([]), array([link(parent)]),
                  bstr(b"\x00\x01"), uint(EPOCH), link(sroot), link(receipts), link(messages), NULL, uint(1_700_000_000 + salt),
                  NULL, uint(0), bstr(b"\x00\x64")]
    child = st.put(header(hdr_fields) if header else array(hdr_fields))
    if root_last:  # the root block moves to the end of the store's (insertion-ordered) table
        st.blocks[root] = st.blocks.pop(root)
    parts = {"child": child, "state_root": sroot, "actors": actors_root, "actor_state": astate, "root": root, "dropped": list(dropped)}
    for d in drop:
        c = parts.get(d, d)
        del st.blocks[c]
        parts["dropped"].append(c)
    claim = {"child_epoch": EPOCH, "child_block_cid": cid_str(child), "parent_state_root": cid_str(sroot), "actor_id": actor_id,
             "actor_state_cid": cid_str(astate), "storage_root": cid_str(root), "slot": hex0x(slot32), "value": hex0x(pad32(value))}
    claim.update(edit(claim, st) if callable(edit) else (edit or {}))
    return st, claim, parts


# ---- the six layouts over one set of (slot, value) pairs -------------------------------------------------------------
def hamt_items(pairs):
    return {k: vec(v) for k, v in pairs}


def layout(kind, pairs, bw=None):
    """→ callable(store) writing the contract-state root of that layout (B1: bit width 5, B2: 3 unless `bw` says otherwise)"""
    if kind == "A1":
        return lambda st: array([bstr(b"p"), array([smap(pairs)])])
    if kind == "A2":
        return lambda st: array([bstr(b""), smap(pairs)])
    if kind == "A3":
        return lambda st: smap(pairs)
    if kind == "B1":
        w = 5 if bw is None else bw
        return lambda st: array([link(pyhamt.build_hamt(st, hamt_items(pairs), w)), uint(w)])
    if kind == "B2":
        w = 3 if bw is None else bw
        return lambda st: cmap([("root", link(pyhamt.build_hamt(st, hamt_items(pairs), w))), ("bitwidth", uint(w))])
    return lambda st: pyhamt._node(st, list(hamt_items(pairs).items()), 0, 5)


S = [slot(i) for i in range(8)]
ABSENT = slot("absent")
VAL = [bytes(range(1, 21)), bytes(5), bytes(range(0xA0, 0xC0)), b"\x7f", bytes(range(200, 240)), b"\x01\x00", b"\xff" * 32, b"\x09" * 3]
PAIRS = list(zip(S, VAL))  # S[1] holds a stored value of all zeros
MANY = PAIRS + [(slot(f"m{i}"), bytes([i + 1, 0x18, 0xFF - i])) for i in range(120)]  # > 32 pointers in a node from width 6 up

CASES = {}  # name → (store, claim, expected status)
META = {}   # name → {"layout", "slot" (present / absent / zero), "trust", "dropped"}


def case(name, expect, root_block, slot32=None, value=None, trust=None, tag=None, **kw):
    assert name not in CASES, name
    salt = int.from_bytes(hashlib.sha256(name.encode()).digest()[:3], "big")
    slot32 = S[0] if slot32 is None else slot32
    value = VAL[0] if value is None else value
    st, claim, parts = chain(root_block, slot32, value, salt=salt, **kw)
    CASES[name] = (st, claim, expect)
    META[name] = {"layout": tag[0] if tag else None, "slot": tag[1] if tag else None, "trust": trust, "dropped": parts["dropped"]}


def raw(b):
    return lambda st: b


# ===== layout sniff (storage/decode.rs:46-96) ==========================================================================
def _well_formed_layouts():
    for L in LAYOUTS:
        case(f"{L.lower()}_present_slot", 1, layout(L, PAIRS), S[2], VAL[2], tag=(L, "present"))
        case(f"{L.lower()}_absent_slot_is_zero", 1, layout(L, PAIRS), ABSENT, b"", tag=(L, "absent"))
        case(f"{L.lower()}_stored_zeros", 1, layout(L, PAIRS), S[1], VAL[1], tag=(L, "zero"))
        case(f"{L.lower()}_present_slot_wrong_value", 21, layout(L, PAIRS), S[2], VAL[3])
        case(f"{L.lower()}_absent_slot_nonzero_claim", 21, layout(L, PAIRS), ABSENT, b"\x01")


_well_formed_layouts()

# decode.rs:47 `vec_sm.into_iter().next()`: only the FIRST map of the list is searched
two_maps = raw(array([bstr(b""), array([smap(PAIRS[:2]), smap(PAIRS[2:])])]))
case("a1_two_maps_slot_only_in_second_is_zero", 1, two_maps, S[2], b"")
case("a1_two_maps_slot_only_in_second_real_value_is_wrong", 21, two_maps, S[2], VAL[2])
case("a1_two_maps_slot_in_first", 1, two_maps, S[0], VAL[0])
# the whole Vec<SmallMap> must decode: a bad second element fails A1; A2/A3/B1/B2 do not fit; C reads `[h'', [map, 7]]` as a
# node whose pointer is a map — neither link nor bucket
case("a1_valid_first_map_malformed_second", 66, raw(array([bstr(b""), array([smap(PAIRS), uint(7)])])))
# decode.rs:47 `if let Some(sm) = …next()`: an empty list falls through; C finds a valid EMPTY node
case("a1_empty_list_is_an_empty_hamt_node", 1, raw(array([bstr(b""), array([])])), S[0], b"")
case("a1_empty_list_nonzero_claim", 21, raw(array([bstr(b""), array([])])), S[0], b"\x01")
# … and `[h'01', []]` falls through to C as well, as a node whose bitfield names a pointer it does not have: what that is depends
# on WHEN the crate compares the two — tests/assumption_cases.py a1_bitfield_01_empty_list_key_on_bit_0 / _on_bit_9

def _inline_maps():
    for L, wrap in (("a2", lambda m: array([bstr(b""), m])), ("a3", lambda m: m)):
        extra = [("a", uint(1))], [("z", array([NULL, cmap([("v", uint(2))])]))]
        case(f"{L}_unknown_field_before_v", 1, raw(wrap(smap(PAIRS, before=extra[0]))))
        case(f"{L}_unknown_field_after_v", 1, raw(wrap(smap(PAIRS, after=extra[1]))))
        # a duplicate "v" is a decode error of THIS attempt; nothing later fits either (C: a map / `[bytes, map]` is no node)
        case(f"{L}_duplicate_v", 66, raw(wrap(smap(PAIRS, after=[("v", array([]))]))))
        case(f"{L}_missing_v", 66, raw(wrap(cmap([("w", array([]))]))))
        case(f"{L}_pair_of_three", 66, raw(wrap(cmap([("v", array([array([bstr(S[0]), bstr(VAL[0]), uint(0)])]))]))))
        case(f"{L}_key_of_31_bytes_is_skipped", 1, raw(wrap(smap([(S[0][:31], b"\x66"), (S[0], VAL[0])]))))
        case(f"{L}_key_of_33_bytes_is_skipped", 1, raw(wrap(smap([(S[0] + b"\0", b"\x66"), (S[0], VAL[0])]))))
        case(f"{L}_only_a_31_byte_prefix_key_is_absent", 1, raw(wrap(smap([(S[0][:31], b"\x66")]))), S[0], b"")
        dup = raw(wrap(smap([(S[3], b"\x01"), (S[0], b"\xaa"), (S[0], b"\xbb")])))
        case(f"{L}_duplicate_key_first_wins", 1, dup, S[0], b"\xaa")
        case(f"{L}_duplicate_key_second_is_wrong", 21, dup, S[0], b"\xbb")
        for n in (0, 1, 31, 32, 33, 64):
            v = bytes((7 * i + n) & 0xFF or 1 for i in range(n))
            case(f"{L}_value_of_{n}_bytes", 1, raw(wrap(smap([(S[4], b"\x01"), (S[0], v)]))), S[0], v)
        case(f"{L}_value_of_33_bytes_first_32_claimed", 21, raw(wrap(smap([(S[0], bytes(range(1, 34)))]))), S[0], bytes(range(1, 33)))


_inline_maps()


def _bit_widths():
    for bw in (1, 3, 5, 6, 7, 8):
        case(f"b1_bit_width_{bw}", 1, layout("B1", MANY, bw), MANY[40][0], MANY[40][1])
        case(f"b1_bit_width_{bw}_absent", 1, layout("B1", MANY, bw), ABSENT, b"")
        case(f"b2_bit_width_{bw}", 1, layout("B2", MANY, bw), MANY[77][0], MANY[77][1])


_bit_widths()


def b1_lying(width_built, width_said):
    return lambda st: array([link(pyhamt.build_hamt(st, hamt_items(MANY), width_built)), uint(width_said)])


# decode.rs:79 `bw as u32` keeps the low 32 bits.  What a width of 0 or 9 is — HAMT_BIT_WIDTH_OUTSIDE_1_TO_8_IS_AN_ERR_OF_THE_GET
# — is stated in tests/assumption_cases.py (b1_bit_width_0, b1_bit_width_9); the truncations to 0, 261 and 259 below lean on it
case("b1_bit_width_2_pow_32_plus_5_truncates_to_5", 1, b1_lying(5, (1 << 32) + 5), MANY[9][0], MANY[9][1])
case("b1_bit_width_2_pow_32_truncates_to_0", 66, b1_lying(5, 1 << 32))
case("b1_bit_width_2_pow_32_plus_261_truncates_to_261", 66, b1_lying(5, (1 << 32) + 261))  # (& 0xff would make it 5)
case("b1_tree_of_width_5_read_at_width_3_misses", 1, b1_lying(5, 3), ABSENT, b"")


def b1_inner_absent(said, b2=False, pairs=PAIRS):
    def root_block(st):
        inner = pyhamt.build_hamt(st, hamt_items(pairs))
        del st.blocks[inner]
        if b2:
            return cmap([("root", link(inner)), ("bitwidth", uint(said))]), [inner]
        return array([link(inner), uint(said)]), [inner]
    return root_block


case("b1_inner_root_absent", 65, b1_inner_absent(5))
# decode.rs:79-80 / :86-87: `load_with_bit_width(&root, store, bw as u32)…?` comes first and fetches the root; nothing has
# looked at the width yet (it is the get on :81 / :88 that uses it) — so an absent inner root is 65 whatever the width says.
# This is the reference's own text, no assumption: the oracle and both HAMT gets of the engine refused the width first (66)
# and were corrected with this case
NOWHERE = PAIRS[:3] + [(slot("in a tree no witness holds"), b"\x01")]  # (so these cases can share the merged witness)
case("b1_bit_width_0_and_inner_root_absent", 65, b1_inner_absent(0, pairs=NOWHERE))
case("b1_bit_width_9_and_inner_root_absent", 65, b1_inner_absent(9, pairs=NOWHERE))
case("b1_bit_width_2_pow_32_and_inner_root_absent", 65, b1_inner_absent(1 << 32, pairs=NOWHERE))
case("b2_bitwidth_0_and_inner_root_absent", 65, b1_inner_absent(0, b2=True, pairs=NOWHERE))
case("b2_bitwidth_9_and_inner_root_absent", 65, b1_inner_absent(9, b2=True, pairs=NOWHERE))
# … while a width out of range over a root that is there but is no node is 66 either way
case("b1_bit_width_9_and_inner_root_undecodable", 66, lambda st: array([link(st.put(b"\xff b1 inner")), uint(9)]))
# a 3-tuple is no MapTuple; at C an array of 3 is no node
case("b1_as_a_3_tuple", 66, lambda st: array([link(pyhamt.build_hamt(st, hamt_items(PAIRS))), uint(5), uint(0)]))
case("b1_inner_root_linked_by_sha256_cid", 1,
     lambda st: array([link(st.put(pyhamt._node(st, list(hamt_items(PAIRS).items()), 0, 5), sha256_cid=True)), uint(5)]), S[2], VAL[2])
case("storage_root_itself_under_a_sha256_cid", 1, layout("C", PAIRS), S[2], VAL[2], root_sha256=True)


def b2(fields):
    """fields: callable(inner root link) → [(name, encoded)]"""
    return lambda st: cmap(fields(link(pyhamt.build_hamt(st, hamt_items(PAIRS), 3))))


case("b2_root_then_bitwidth", 1, b2(lambda r: [("root", r), ("bitwidth", uint(3))]))
case("b2_bitwidth_then_root", 1, b2(lambda r: [("bitwidth", uint(3)), ("root", r)]))
case("b2_extra_keys", 1, b2(lambda r: [("a", NULL), ("root", r), ("m", cmap([("root", uint(1))])), ("bitwidth", uint(3)), ("z", array([]))]))
# a failed B2 falls to C, where a map is no node
case("b2_duplicate_root", 66, b2(lambda r: [("root", r), ("bitwidth", uint(3)), ("root", r)]))
case("b2_duplicate_bitwidth", 66, b2(lambda r: [("root", r), ("bitwidth", uint(3)), ("bitwidth", uint(3))]))
case("b2_only_root", 66, b2(lambda r: [("root", r)]))
case("b2_bitwidth_negative", 66, b2(lambda r: [("root", r), ("bitwidth", nint(-3))]))
case("b2_bitwidth_2_pow_32_plus_3_truncates_to_3", 1, b2(lambda r: [("root", r), ("bitwidth", uint((1 << 32) + 3))]))
case("b2_bitwidth_2_pow_32_plus_259_truncates_to_259", 66, b2(lambda r: [("root", r), ("bitwidth", uint((1 << 32) + 259))]))  # (& 0xff: 3)
# decode.rs:68 comes before :85 — a MapStruct that also has a "v" field IS a SmallMap (A3), its HAMT is never opened
case("b2_with_a_v_field_is_taken_by_a3", 1, b2(lambda r: [("root", r), ("bitwidth", uint(3)), ("v", array([]))]), S[0], b"")
case("b2_with_a_v_field_real_value_is_wrong", 21, b2(lambda r: [("root", r), ("bitwidth", uint(3)), ("v", array([]))]), S[0], VAL[0])

case("c_root_absent", 65, layout("C", PAIRS), drop=["root"])
case("c_root_is_an_empty_node", 1, raw(node(0, [])), S[0], b"")
B3 = sorted(slot_with_index(17, k) for k in range(3))
B4 = sorted(slot_with_index(17, k) for k in range(4))
bucket3 = raw(node(1 << 17, [bucket([(k, vec(bytes([i + 1]) * 4)) for i, k in enumerate(B3)])]))
case("c_bucket_of_3_key_first", 1, bucket3, B3[0], b"\x01" * 4)
case("c_bucket_of_3_key_middle", 1, bucket3, B3[1], b"\x02" * 4)
case("c_bucket_of_3_key_last", 1, bucket3, B3[2], b"\x03" * 4)
case("c_bucket_of_3_other_key_same_index_is_absent", 1, bucket3, slot_with_index(17, 3), b"")
# a bucket of 4, an unsorted bucket: HAMT_BUCKET_SIZE_AND_ORDER_ARE_NOT_CHECKED_ON_READ — tests/assumption_cases.py
# c_bucket_of_4_fourth_key, c_bucket_unsorted
# serde decodes the whole node: a bad value in ANOTHER bucket is the node's decode error
case("c_bad_value_in_another_bucket", 66, raw(node((1 << 17) | (1 << 3), [bucket([(slot_with_index(3), bstr(b"\x01"))]), bucket([(B3[0], vec(b"\x01"))])])), B3[0], b"\x01")
case("c_two_buckets_rank_1", 1, raw(node((1 << 17) | (1 << 3), [bucket([(slot_with_index(3), vec(b"\x09"))]), bucket([(B3[0], vec(b"\x01"))])])), B3[0], b"\x01")
case("c_child_link_missing", 65, raw(node(1 << 17, [link(OTHER)])), B3[0], b"")
case("c_child_link_missing_key_elsewhere_is_zero", 1, raw(node(1 << 17, [link(OTHER)])), slot_with_index(4), b"")


def deep_chain(st):
    """33 hand-linked nodes at bit width 8 along one key's path: 32 levels use all 256 hash bits, the 33rd node is decoded
    and `HashBits::next` then fails — fvm_ipld_hamt's MaxDepth, status 70, on every judge."""
    h = hashlib.sha256(S[0]).digest()
    nd = node(0, [])
    for d in range(31, -1, -1):
        nd = node(1 << h[d], [link(st.put(nd))])
    return array([link(st.put(nd)), uint(8)])


case("c_chain_deeper_than_the_hash_bits_at_width_8", 70, deep_chain, S[0], b"")
case("c_chain_deeper_than_the_hash_bits_other_key_is_zero", 1, deep_chain, S[1], b"")

# ===== value spellings behind a HAMT (Vec<u8>: a CBOR array of uints ≤ 255) =====================================================
FILLS = {
    "all_17": lambda n: bytes([0x17] * n),
    "all_18": lambda n: bytes([0x18] * n),                        # every element in its two-byte spelling
    "alternating_17_ff": lambda n: bytes([0x17, 0xFF] * n)[:n],
    "leading_zero": lambda n: (b"\0" + bytes((0x80 + i) & 0xFF for i in range(n)))[:n],
}


def value_node(encoded_value, key=None):
    """A width-5 node with three buckets; the one in the middle holds `key` → the value as spelled"""
    key = S[0] if key is None else key
    items = {S[5]: vec(VAL[5]), key: encoded_value, S[6]: vec(VAL[6])}
    return lambda st: pyhamt._node(st, list(items.items()), 0, 5)


def _element_counts():
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 23, 24, 31, 32, 33, 35, 36, 40, 64, 255, 256, 300):
        for fill, f in FILLS.items():
            case(f"value_{n}_elements_{fill}", 1, value_node(vec(f(n))), S[0], f(n))


_element_counts()
case("value_33_elements_first_32_claimed_is_wrong", 21, value_node(vec(bytes(range(1, 34)))), S[0], bytes(range(1, 33)))
case("value_32_elements_last_differs", 21, value_node(vec(bytes(range(1, 33)))), S[0], bytes(range(1, 32)) + b"\x00")
five = bytes([5, 0x18, 0, 0xFF, 7])
case("value_header_98_05", 1, value_node(b"\x98\x05" + b"".join(uint(x) for x in five)), S[0], five)
case("value_header_99_00_05", 1, value_node(b"\x99\x00\x05" + b"".join(uint(x) for x in five)), S[0], five)
case("value_elements_18_05", 1, value_node(head(4, 5) + b"\x18\x05" * 5), S[0], b"\x05" * 5)
case("value_elements_19_00_05", 1, value_node(head(4, 5) + b"\x19\x00\x05" * 5), S[0], b"\x05" * 5)
case("value_elements_19_00_05_among_plain_ones_at_33", 1, value_node(head(4, 33) + b"\x01" * 16 + b"\x19\x00\x05" + b"\x18\xee" * 16), S[0],
     b"\x01" * 16 + b"\x05" + b"\xee" * 16)
case("value_element_256", 66, value_node(array([uint(1), uint(256)])))
case("value_element_minus_1", 66, value_node(array([uint(1), nint(-1)])))
case("value_is_a_byte_string", 66, value_node(bstr(b"\x01\x02")))
case("value_is_an_indefinite_array", 66, value_node(b"\x9f\x01\x02\xff"))
case("value_element_is_a_float64", 66, value_node(array([b"\xfb" + bytes(8)])))
# The value is the final bytes of its block and ends exactly on a 128-byte line.  The engine lays every block on a line of
# its own (csrc/host/witness.cpp, by its schedule: `root_last` orders the host table only), so the staged read of the tabled
# route — 80 bytes from the value's first byte, 46 of them past this 34-byte value — leaves the block's own line: it runs
# into whatever the arena holds next, another block, or the 256 bytes of kTailSlack the arena ends with, which cover it.
def _value_ending_on_a_line():
    v = bytes(range(1, 0x18)) + bytes(range(1, 10))  # 32 one-byte elements: `98 20` + 32 = 34 bytes
    filler = (slot_with_index(3), vec(bytes(range(1, 16))))  # an earlier bucket that pads the block to 128 bytes
    block = node((1 << 17) | (1 << 3), [bucket([filler]), bucket([(B3[0], vec(v))])])
    assert len(block) == 128 and block.endswith(vec(v))
    case("value_at_the_very_end_of_a_block_that_ends_on_a_128_byte_line", 1, raw(block), B3[0], v, root_last=True)
    case("value_at_the_very_end_of_a_block_last_byte_differs", 21, raw(block), B3[0], v[:-1] + b"\x7f", root_last=True)


_value_ending_on_a_line()

# ===== typed decodes (common/decode.rs, fvm_shared) ======================================================================
C5 = layout("C", PAIRS)
case("evm_v6_optional_fields_null", 1, C5)
case("evm_v6_reserved_is_a_map_tombstone_a_link", 1, C5, evm=lambda f: array(f[:3] + [cmap([("a", uint(1))]), f[4], link(OTHER)]))
# six fields with an int in the 4th: Option<IgnoredAny> takes it, the 6-tuple attempt succeeds (decode.rs:81)
case("evm_v6_shape_with_an_int_as_4th_field_is_a_v6", 1, C5, evm=lambda f: array(f[:3] + [uint(7), f[4], NULL]))
case("evm_v5_tombstone_null", 1, C5, evm=lambda f: array(f[:3] + [f[4], NULL]))
case("evm_v5_tombstone_an_int", 1, C5, evm=lambda f: array(f[:3] + [f[4], uint(3)]))
# five fields with null where V5 has its nonce: too short for V6, and no u64 for V5 (decode.rs:89-90)
case("evm_5_fields_with_a_null_4th_is_neither", 66, C5, evm=lambda f: array(f[:3] + [NULL, f[4]]))
case("evm_bytecode_hash_of_31_bytes", 66, C5, evm=lambda f: array([f[0], bstr(bytes(31))] + f[2:]))
case("evm_bytecode_hash_of_33_bytes", 66, C5, evm=lambda f: array([f[0], bstr(bytes(33))] + f[2:]))
case("evm_nonce_negative", 66, C5, evm=lambda f: array(f[:4] + [nint(-1), f[5]]))
case("evm_nonce_a_float64", 66, C5, evm=lambda f: array(f[:4] + [b"\xfb\x44" + bytes(7), f[5]]))  # (a uint head cannot exceed u64)
# a nonce larger than u64 has no uint spelling; what CBOR offers for it is a bignum, tag 2 over its big-endian bytes — DAG-CBOR
# knows tag 42 only, so the block does not decode at all
case("evm_nonce_2_pow_64_as_a_bignum", 66, C5, evm=lambda f: array(f[:4] + [b"\xc2" + bstr(b"\x01" + bytes(8)), f[5]]))
case("evm_nonce_u64_max", 1, C5, evm=lambda f: array(f[:4] + [uint((1 << 64) - 1), f[5]]))
case("evm_4_fields", 66, C5, evm=lambda f: array(f[:4]))
case("evm_7_fields", 66, C5, evm=lambda f: array(f + [NULL]))
case("evm_contract_state_null", 66, C5, evm=lambda f: array(f[:2] + [NULL] + f[3:]))
case("state_root_version_0", 1, C5, state_root=lambda f: array([uint(0)] + f[1:]))
case("state_root_version_5", 1, C5)
case("state_root_version_6", 66, C5, state_root=lambda f: array([uint(6)] + f[1:]))
case("state_root_2_fields", 66, C5, state_root=lambda f: array(f[:2]))
case("state_root_4_fields", 66, C5, state_root=lambda f: array(f + [NULL]))
case("state_root_info_null", 66, C5, state_root=lambda f: array(f[:2] + [NULL]))
case("actor_state_4_fields", 66, C5, actor=lambda f: array(f[:4]))
case("actor_state_6_fields", 66, C5, actor=lambda f: array(f + [NULL]))
case("actor_state_delegated_address_present", 1, C5, actor=lambda f: array(f[:4] + [bstr(b"\x04\x0a" + bytes(range(20)))]))
case("actor_state_balance_empty_bytes", 1, C5, actor=lambda f: array(f[:3] + [bstr(b""), f[4]]))
case("actor_state_balance_an_int", 66, C5, actor=lambda f: array(f[:3] + [uint(5), f[4]]))
case("header_15_fields", 66, C5, header=lambda f: array(f[:15]))
case("header_17_fields", 66, C5, header=lambda f: array(f + [NULL]))
case("header_negative_height", 1, C5, header=lambda f: array(f[:7] + [nint(-5)] + f[8:]))
case("header_parents_empty", 1, C5, header=lambda f: array(f[:5] + [array([])] + f[6:]))
case("header_parent_state_root_null", 66, C5, header=lambda f: array(f[:8] + [NULL] + f[9:]))
case("header_timestamp_negative", 66, C5, header=lambda f: array(f[:12] + [nint(-1)] + f[13:]))
case("header_trailing_byte", 66, C5, header=lambda f: array(f) + b"\x00")

# ===== the claim's strings =================================================================================================
case("claim_child_cid_garbage", 69, C5, edit={"child_block_cid": "garbage"})
case("claim_slot_without_0x", 1, C5, edit={"slot": S[0].hex()})
case("claim_slot_0x0x", 1, C5, edit={"slot": "0x0x" + S[0].hex()})
case("claim_slot_upper_case_hex", 1, C5, edit={"slot": "0x" + S[0].hex().upper()})
case("claim_slot_of_2_bytes", 69, C5, edit={"slot": "0x1234"})
case("claim_slot_of_33_bytes", 69, C5, edit={"slot": "0x" + S[0].hex() + "00"})
case("claim_value_upper_case", 1, C5, edit={"value": "0x" + pad32(VAL[0]).hex().upper()})
case("claim_value_0X_prefix", 1, C5, edit={"value": "0X" + pad32(VAL[0]).hex()})
case("claim_value_without_0x", 21, C5, edit={"value": pad32(VAL[0]).hex()})
case("claim_value_short", 21, C5, edit={"value": hex0x(VAL[0])})
case("claim_untrusted_epoch", 3, C5, trust=TRUST_WINDOW, edit={"child_epoch": 5})
case("claim_trusted_epoch_at_the_window_edge", 1, C5, trust=TRUST_WINDOW, edit={"child_epoch": 1100})


def _upper(name):
    """the named CID string of a valid chain, re-spelled in multibase B (upper-case base32): parses, equals no to_string()"""
    return lambda claim, st: {name: "B" + claim[name][1:].upper()}


case("claim_state_root_in_multibase_upper", 18, C5, edit=_upper("parent_state_root"))
case("claim_actor_state_in_base16", 19, C5, edit=lambda c, st: {"actor_state_cid": "f" + pystorage.cid_from_string(c["actor_state_cid"]).hex()})
case("claim_storage_root_in_multibase_upper", 20, C5, edit=_upper("storage_root"))
case("claim_child_cid_in_multibase_upper_is_the_same_cid", 1, C5, edit=_upper("child_block_cid"))
case("claim_storage_root_other", 20, C5, edit={"storage_root": cid_str(OTHER)})
case("claim_actor_not_in_the_tree", 68, C5, edit={"actor_id": 999})
case("claim_other_actor_of_the_tree", 19, C5, edit={"actor_id": 1002})

# ===== two defects in one chain: the earlier step's status comes out =======================================================
# steps: trust → header → state-root compare → StateRoot decode → actor get → actor-state compare → EVM decode →
#        storage-root compare → slot parse → root kind → value
BAD = b"\xff"  # no DAG-CBOR item
case("two_unparsable_child_cid_and_untrusted_epoch", 69, C5, trust=TRUST_WINDOW, edit={"child_epoch": 5, "child_block_cid": "garbage"})
case("two_untrusted_epoch_and_header_missing", 3, C5, trust=TRUST_WINDOW, drop=["child"], edit={"child_epoch": 5})
case("two_header_missing_and_state_root_mismatch", 65, C5, drop=["child"], edit={"parent_state_root": cid_str(OTHER)})
case("two_header_undecodable_and_state_root_mismatch", 66, C5, header=lambda f: BAD, edit={"parent_state_root": cid_str(OTHER)})
case("two_header_missing_and_bad_slot_hex", 65, C5, drop=["child"], edit={"slot": "0xzz"})


# the claim names a block that IS in the witness and is no StateRoot; the header names the real one
case("two_state_root_mismatch_and_state_root_undecodable", 18, C5,
     edit=lambda c, st: {"parent_state_root": cid_str(st.put(BAD + b"two_state_root"))})
case("two_state_root_undecodable_and_actor_not_found", 66, C5, state_root=lambda f: BAD, edit={"actor_id": 999})
case("two_state_root_missing_and_actor_state_mismatch", 65, C5, drop=["state_root"], edit={"actor_state_cid": cid_str(OTHER)})
case("two_actors_root_missing_and_actor_state_mismatch", 65, C5, drop=["actors"], edit={"actor_state_cid": cid_str(OTHER)})
case("two_actor_not_found_and_actor_state_mismatch", 68, C5, edit={"actor_id": 999, "actor_state_cid": cid_str(OTHER)})
case("two_actor_not_found_and_evm_state_missing", 68, C5, drop=["actor_state"], edit={"actor_id": 999})
case("two_actor_state_mismatch_and_evm_state_missing", 19, C5, edit={"actor_state_cid": cid_str(OTHER)})
case("two_actor_state_mismatch_and_evm_state_undecodable", 19, C5, evm=lambda f: BAD, edit={"actor_id": 1002})
case("two_evm_state_undecodable_and_storage_root_mismatch", 66, C5, evm=lambda f: BAD, edit={"storage_root": cid_str(OTHER)})
case("two_evm_state_missing_and_storage_root_mismatch", 65, C5, drop=["actor_state"], edit={"storage_root": cid_str(OTHER)})
case("two_storage_root_mismatch_and_bad_slot_hex", 20, C5, edit={"storage_root": cid_str(OTHER), "slot": "0x12"})
case("two_storage_root_mismatch_and_storage_root_absent", 20, C5, edit={"storage_root": cid_str(OTHER)})
case("two_bad_slot_hex_and_storage_root_absent", 69, C5, drop=["root"], edit={"slot": "0x12"})
case("two_bad_slot_hex_and_storage_root_undecodable", 69, raw(BAD), edit={"slot": "0x12"})
case("two_storage_root_absent_and_wrong_value", 65, C5, drop=["root"], edit={"value": hex0x(bytes(32))})
case("two_storage_root_undecodable_and_wrong_value", 66, raw(BAD), edit={"value": hex0x(bytes(32))})
case("two_value_undecodable_and_wrong_value", 66, value_node(bstr(b"\x01")), edit={"value": hex0x(bytes(32))})
case("two_evm_state_undecodable_and_bad_slot_hex", 66, C5, evm=lambda f: BAD, edit={"slot": "0x12"})


# ===== the cases that state an assumption about the crates live in tests/assumption_cases.py; they run in this table too ==
def _assumption_cases():
    import assumption_cases as ac

    for name in ac.STORAGE_CASES:
        assert name not in CASES, name
        st, claim, expect, dropped = ac.STORAGE_CASES[name](parts=True)
        CASES[name] = (st, claim, expect)
        META[name] = {"layout": None, "slot": None, "trust": None, "dropped": dropped}


_assumption_cases()

# The packed claim row (include/ipcfp.h ipcfp_storage_claim_t) carries CIDs and 32-byte words, no strings: it can express a
# claim only where every string is its canonical spelling, and marks what it cannot (flags != 63) for the string route.
# These are the cases it declines, and no other — each edits a claim string to a spelling the verifier COMPARES as a string
# (a CID string against a to_string(), the value's prefix) or cannot parse.  Spellings the verifier only parses, trims or
# compares without case — the child CID in another multibase, "0x0x" before the slot, "0X" before the value — fit the row.
PACKED_MAY_DECLINE = frozenset({
    "claim_child_cid_garbage", "claim_slot_of_2_bytes", "claim_slot_of_33_bytes",
    "claim_value_without_0x", "claim_value_short",
    "claim_state_root_in_multibase_upper", "claim_actor_state_in_base16", "claim_storage_root_in_multibase_upper",
    "two_unparsable_child_cid_and_untrusted_epoch", "two_header_missing_and_bad_slot_hex",
    "two_storage_root_mismatch_and_bad_slot_hex", "two_bad_slot_hex_and_storage_root_absent",
    "two_bad_slot_hex_and_storage_root_undecodable", "two_evm_state_undecodable_and_bad_slot_hex",
})


# ---- helpers the two test files share ------------------------------------------------------------------------------------
def merged(names=None):
    """All cases in ONE witness (CIDs are content hashes: stores merge by dict union).  A case that needs a CID absent
    which another case holds — or different bytes under one CID — stays in a witness of its own.
    → (store, [names merged, in table order], [names kept apart])"""
    st = pyamt.Store()
    absent, inn, out = set(), [], []
    for name in (names or CASES):
        blocks = CASES[name][0].blocks
        dropped = META[name]["dropped"]
        if any(c in absent or st.blocks.get(c, b) != b for c, b in blocks.items()) or any(c in st.blocks for c in dropped):
            out.append(name)
            continue
        st.blocks.update(blocks)
        absent.update(dropped)
        inn.append(name)
    return st, inn, out


def proofs(claim_list):
    """claim dicts → an object with .arr (ctypes ipcfp_storage_proof_t[n]) and .n, owning the strings"""
    import types

    import claims

    arr = (claims.StorageProof * max(len(claim_list), 1))()
    keep = []
    for p, c in zip(arr, claim_list):
        p.child_epoch = c["child_epoch"]
        p.actor_id = c["actor_id"]
        for f in ("child_block_cid", "parent_state_root", "actor_state_cid", "storage_root", "slot", "value"):
            b = c[f].encode()
            keep.append(b)
            setattr(p, f, b)
    return types.SimpleNamespace(arr=arr, n=len(claim_list), _keep=keep)


def trust_policy(t):
    import claims

    return None if t is None else claims.TrustPolicy(kind=1, ec_chain_empty=t[0], min_epoch=t[1], max_epoch=t[2])


# ---- the structured mutator ---------------------------------------------------------------------------------------------------
def encode(x) -> bytes:
    """a pystorage tree → minimal DAG-CBOR; `Raw` leaves are written as they are"""
    if type(x) is Raw:
        return x.b
    if x is None:
        return NULL
    if x is True or x is False:
        return b"\xf5" if x else b"\xf4"
    if type(x) is int:
        return uint(x) if x >= 0 else nint(x)
    if type(x) is bytes:
        return bstr(x)
    if type(x) is str:
        return text(x)
    if type(x) is list:
        return array([encode(e) for e in x])
    if type(x) is pystorage.Link:
        return link(x.cid)
    if type(x) is pystorage.Map:
        return head(5, len(x.entries)) + b"".join(encode(k) + encode(v) for k, v in x.entries)
    raise TypeError(type(x))


class Raw:
    def __init__(self, b):
        self.b = b


def _paths(x, at=()):
    yield at
    if type(x) is list:
        for i, e in enumerate(x):
            yield from _paths(e, at + (i,))
    elif type(x) is pystorage.Map:
        for i, (_k, v) in enumerate(x.entries):
            yield from _paths(v, at + (i,))


def _get(x, path):
    for i in path:
        x = x[i] if type(x) is list else x.entries[i][1]
    return x


def _set(x, path, new):
    if not path:
        return new
    parent = _get(x, path[:-1])
    if type(parent) is list:
        parent[path[-1]] = new
    else:
        parent.entries[path[-1]] = (parent.entries[path[-1]][0], new)
    return x


def _long_head(b: bytes) -> bytes:
    """the item's head re-spelled one width class wider than it is (non-minimal)"""
    major, info = b[0] >> 5, b[0] & 31
    if major == 7 or info >= 27:
        return b
    if info < 24:
        return bytes([(major << 5) | 24, info]) + b[1:]
    nb = 1 << (info - 24)
    return bytes([(major << 5) | (info + 1)]) + bytes(nb) + b[1:]


def mutate_field(tree, rng, cids):
    """One field of the tree re-spelled from the menu: wrong major type, length ± 1, null, non-minimal head, swapped link."""
    paths = list(_paths(tree))
    links = [p for p in paths if type(_get(tree, p)) is pystorage.Link]
    if links and rng.integers(2):  # half of the time a link, where the block has one: the compares of the chain hang on them
        paths = links
    path = paths[int(rng.integers(len(paths)))]
    old = _get(tree, path)
    kind = int(rng.integers(5))
    if type(old) is pystorage.Link and rng.integers(4):
        kind = 4
    if kind == 0:  # wrong major type
        new = Raw(uint(len(old))) if type(old) in (bytes, str) else Raw(bstr(b"\x01"))
    elif kind == 1:  # length ± 1
        grow = bool(rng.integers(2))
        if type(old) is list:
            new = old + [0] if grow else old[:-1]
        elif type(old) in (bytes, str):
            new = old + (b"\0" if type(old) is bytes else "0") if grow else old[:-1]
        elif type(old) is int:
            new = old + 1 if grow else old - 1
        else:
            new = Raw(encode(old) + b"\x00") if grow else Raw(encode(old)[:-1])
    elif kind == 2:
        new = None
    elif kind == 3:
        new = Raw(_long_head(encode(old)))
    else:  # a link to another block of the chain (any field may become one)
        new = pystorage.Link(cids[int(rng.integers(len(cids)))])
    return _set(tree, path, new)


def mutated_chain(rng):
    """A valid chain of a random layout with one or two fields of random blocks re-spelled (nothing is re-hashed: the store
    keeps the new bytes under the old CID), or a block dropped; a random slot kind; sometimes a trust window.
    → (blocks dict, claim, trust)"""
    L = LAYOUTS[int(rng.integers(6))]
    pairs = PAIRS if rng.integers(3) else MANY[: int(rng.integers(9, 60))]
    k = int(rng.integers(len(pairs) + 1))
    s, v = (ABSENT, b"") if k == len(pairs) else pairs[k]
    st, claim, _ = chain(layout(L, pairs), s, v, salt=int(rng.integers(1 << 20)), n_actors=int(rng.integers(1, 4)))
    blocks = st.blocks
    cids = list(blocks)
    for _ in range(int(rng.integers(1, 3))):
        c = cids[int(rng.integers(len(cids)))]
        if c not in blocks:
            continue
        if rng.integers(8) == 0:
            del blocks[c]
            continue
        try:
            tree = pystorage.decode(blocks[c])
        except pystorage.Err:
            continue  # (the first mutation left no tree to edit)
        blocks[c] = encode(mutate_field(tree, rng, cids))
    trust = None
    if rng.integers(6) == 0:
        trust = (0, EPOCH - int(rng.integers(0, 3)), EPOCH + 5) if rng.integers(2) else (int(rng.integers(2)), EPOCH + 1, EPOCH + 9)
    return blocks, claim, trust


def store_of(blocks):
    st = pyamt.Store()
    st.blocks = dict(blocks)
    return st
