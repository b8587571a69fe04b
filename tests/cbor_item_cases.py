"""Single DAG-CBOR items for the reader underneath everything (csrc/kernels/cbor_dev.h), and the CARRIERS that bring one
item in front of each build of that reader.

ROWS is a generated table of `Row(group, name, item bytes, literal verdict)`: the verdict — well-formed or not — is stated by
the rule that writes the row (the named rules of tests/assumption_cases.py), never taken from a
reader.  tests/pystorage.py `decode` (written from the survey, Python's own UTF-8 decoder) must reproduce every verdict,
the C++ oracle must, and every route of the engine must (tests/test_cbor_items.py, tests/test_gpu_cbor_items.py).

From the table two sweeps are derived, as `Case(name, group, at, item, ok)`:

  residues    every row sits at block offset ≡ its number (mod 16); a subset (one item per head width, items with an
              8-byte argument, strings and texts of 7 to 17 bytes, every link form) sits at all 16 residues and at every
              offset from 112 to 143, across a 128-byte line.  `at` < 16 is a residue, `at` ≥ 16 an offset; the padding
              is a byte string in front of the item, inside the carrier block.
  block end   every proper prefix of every well-formed item of at most 64 bytes as the LAST bytes of its carrier block
              (which is then malformed), and the whole item followed by one byte more.  LAST_BLOCK takes a part of them
              once more with the carrier block as the last block of the arena's schedule, so that a look-ahead has
              nothing but the arena's tail behind it.

CARRIER → KERNEL → READER BUILD (each route read in the source):

  amt        AMT leaf value, kind `any`, Amtv0 (width 3, height ≥ 1) and v3 (width 5) → ipcfp_amt_get → k_amt_get
             (walk.hip) → walk_dev.h check_value → Rd::skip, the plain 16-byte window (IPCFP_LINE_STAGE 0).  One case
             per leaf `[bitmap, [], [pad, item]]`; a malformed leaf fails its own indices only.
  hamt       HAMT bucket value, kind `any`, one case per leaf node of a width-5 tree two link levels deep →
             ipcfp_hamt_get: the walker (walk.hip k_hamt_get, plain window), level by level (hamt_levels.hip: the plain
             window, its one-lane parse hamt_table_body.h `value_kinds` → skip), the whole-witness node table
             (hamt_table_lane.hip: IPCFP_LINE_STAGE 2, the re-aimed window, `ensure_span`, `value_kinds` → skip).  The
             leaf is `[bitfield, [[[pad key, filler], [key, item]]]]`: the padding is the KEY of a first entry.
  typed      the same two carriers with kind `vec_u8`, `receipt`, `cid` and (block end only) `actor_state`: check_vec_u8
             and its 8-byte fetch guard, HamtTableEntry's `82 58 20` fast entry and vec_u8_end (the case keys are 32 bytes
             long for that), check_receipt, read_link's 43-byte fast path, actor_entry_fast's length guard.  Padding is a
             value of the same kind in front (a Vec<u8> of zeros), the pad key in a HAMT, the receipt's own return data.
  header     field 0 (the first item) and field 15 (the last item) of a child header, both skipped by header_dev.h → the
             event verifier's tipset prologue out of LDS (tipset_prepare.hip: IPCFP_RD_LDS 1, the second head / at /
             peek64 / text_ok) while the header is under the 8 KB stage, the general reader over it
             (tipset_prepare_general.hip, open_block_staged) once a pad in field 13 lifts it over; and
             ipcfp_verify_storage_proofs' header decode (verify_storage.hip, the plain window).  HEADER_ROWS says which
             part of the table goes there and why.

No carrier drops a row: the longest item (a map of 256 pairs, 771 bytes) fits a leaf of either tree, so the share of the
table a carrier cannot hold is 0 (asserted in tests/test_cbor_items.py)."""
import collections
import functools
import hashlib

import pyamt
import pyhamt
from pyamt import NULL, array, bstr, head, link, uint
from storage_chain_cases import cmap, nint, text

TRUE, NOT_FOUND, DECODE = 1, 32, 66
Row = collections.namedtuple("Row", "group name item ok")
Case = collections.namedtuple("Case", "name group at item ok")
ROWS = []
_names = set()

STD = pyamt.cid_of(b"a block some link names")  # the standard 38-byte CID
DIGEST = hashlib.sha256(b"digest").digest()
V0 = b"\x12\x20" + DIGEST


def row(group, name, item, ok):
    assert name not in _names, name
    _names.add(name)
    ROWS.append(Row(group, name, bytes(item), bool(ok)))


def spell(major, n, nb):
    """an item head with its argument in nb bytes (0: in the initial byte)"""
    if nb == 0:
        assert n < 24
        return bytes([(major << 5) | n])
    return bytes([(major << 5) | {1: 24, 2: 25, 4: 26, 8: 27}[nb]]) + n.to_bytes(nb, "big")


def body_for(major, n):
    """what follows a head of `major` with argument n → (bytes, the item is well-formed): the whole body up to 256, three
    bytes of one (a body cut short) past it"""
    whole = n <= 256
    if major < 2:
        return b"", True
    if major == 2:
        return bytes((37 * i + n) & 0xFF for i in range(n if whole else 3)), whole
    if major == 3:
        return bytes(0x20 + (7 * i + n) % 0x5F for i in range(n if whole else 3)), whole
    if major == 4:
        return b"\x00" * (n if whole else 3), whole
    if major == 5:
        return b"\x61k\x00" * (n if whole else 1), whole
    return bstr(b"\x00" + STD), n == 42  # the only tag is 42


# ===== heads ====================================================================================================================
EDGES = (23, 24, 255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1)


def _heads():
    for m in range(7):
        for nb in (0, 1, 2, 4, 8):
            for n in sorted({3, 42} | set(EDGES)):  # (3 and 42: a small value, non-minimal in every width but the first)
                if (nb == 0 and n >= 24) or (nb and n >> (8 * nb)):
                    continue
                body, ok = body_for(m, n)
                row("heads", f"major{m}_arg_{n}_in_{nb}_bytes", spell(m, n, nb) + body, ok)
    for m in range(8):
        for ai in (28, 29, 30, 31):
            row("heads", f"major{m}_additional_info_{ai}", bytes([(m << 5) | ai]), False)
            row("heads", f"major{m}_additional_info_{ai}_over_an_item_and_a_break", bytes([(m << 5) | ai]) + b"\x00\xff", False)


_heads()


# ===== major 7 ==================================================================================================================
def _major7():
    for v in range(24):
        row("major7", f"simple_{v}", bytes([0xE0 | v]), v in (20, 21, 22))  # false, true, null
    for x in (0, 20, 22, 32, 255):
        row("major7", f"simple_in_one_byte_{x}", bytes([0xF8, x]), False)
    row("major7", "float16", b"\xf9\x3c\x00", False)
    row("major7", "float32", b"\xfa\x3f\x80\x00\x00", False)
    for tag, payload in (("one", bytes.fromhex("3ff0000000000000")), ("nan", bytes.fromhex("7ff8000000000000")), ("zero", bytes(8)),
                         ("all_ones", b"\xff" * 8)):
        row("major7", f"float64_{tag}", b"\xfb" + payload, True)
    row("major7", "break", b"\xff", False)


_major7()


# ===== strings ==================================================================================================================
STRING_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 255, 256)


def _strings():
    for major, what in ((2, "bytes"), (3, "text")):
        for n in STRING_LENGTHS:
            body, _ = body_for(major, n)
            row("strings", f"{what}_of_{n}", head(major, n) + body, True)
            if n:
                row("strings", f"{what}_of_{n}_one_byte_short", head(major, n) + body[:-1], False)
        # a length that only fits 64 bits over a short body; 2^32 + 3 is 3 to a reader that keeps 32 bits of it
        for n in (1 << 31, (1 << 32) - 1):
            row("strings", f"{what}_length_{n}_over_3_bytes", spell(major, n, 4) + b"abc", False)
        for n in (1 << 32, (1 << 32) + 3, 1 << 63, (1 << 64) - 1):
            row("strings", f"{what}_length_{n}_over_3_bytes", spell(major, n, 8) + b"abc", False)


_strings()


# ===== UTF-8 ====================================================================================================================
# the literal verdict of each sequence, by the definition of UTF-8 (RFC 3629: shortest form, no surrogates, at most U+10FFFF)
UTF8 = [
    ("c0_80", "c080", False), ("c1_bf", "c1bf", False), ("c2_80", "c280", True), ("df_bf", "dfbf", True),
    ("e0_80_80", "e08080", False), ("e0_9f_bf", "e09fbf", False), ("e0_a0_80", "e0a080", True), ("ed_9f_bf", "ed9fbf", True),
    ("ed_a0_80", "eda080", False), ("ed_bf_bf", "edbfbf", False), ("ee_80_80", "ee8080", True), ("ef_bf_bf", "efbfbf", True),
    ("f0_80_80_80", "f0808080", False), ("f0_8f_bf_bf", "f08fbfbf", False), ("f0_90_80_80", "f0908080", True),
    ("f4_8f_bf_bf", "f48fbfbf", True), ("f4_90_80_80", "f4908080", False), ("f5_80_80_80", "f5808080", False),
    ("f8_88_80_80_80", "f888808080", False),
    ("lone_80", "80", False), ("lone_bf", "bf", False), ("c3_then_ascii", "c328", False), ("e2_then_ascii", "e228a1", False),
    ("e2_82_then_ascii", "e28228", False), ("f0_then_ascii", "f0288cbc", False), ("f0_9f_98_then_ascii", "f09f9828", False),
    ("c3_cut_off", "c3", False), ("e2_82_cut_off", "e282", False), ("f0_9f_98_cut_off", "f09f98", False),
]
UTF8_TOTALS = (8, 9, 17, 20)  # total text lengths: one at text_ok's `len <= 8`, the others past it


def _utf8():
    for name, hx, ok in UTF8:
        seq = bytes.fromhex(hx)
        n = len(seq)
        row("utf8", f"{name}_alone", head(3, n) + seq, ok)
        for total in UTF8_TOTALS:
            places = {"first": 0, "middle": (total - n) // 2, "last": total - n}
            if total == 20:  # … and across the 8th and the 16th byte of the text
                places.update({"over_byte_8": 8 - max(1, n - 1), "over_byte_16": 16 - max(1, n - 1)})
            for where, at in places.items():
                body = b"a" * at + seq + b"z" * (total - at - n)
                assert len(body) == total
                row("utf8", f"{name}_{where}_of_{total}", head(3, total) + body, ok)


_utf8()


# ===== arrays and maps ==========================================================================================================
def nested(depth, inner):
    """arrays and maps nested into each other, `inner` at the bottom"""
    x = inner
    for d in range(depth):
        x = array([x]) if (depth - d) % 2 else cmap([("k", x)])
    return x


def _containers():
    G = "containers"
    for n in (0, 1, 23, 24, 256):
        row(G, f"array_of_{n}", head(4, n) + b"\x00" * n, True)
        row(G, f"map_of_{n}", head(5, n) + b"\x61k\x00" * n, True)
    # the count against the bytes that remain (the item is the last of its block)
    row(G, "array_count_3_over_3_bytes", b"\x83\x00\x00\x00", True)
    row(G, "array_count_4_over_3_bytes", b"\x84\x00\x00\x00", False)
    row(G, "array_count_24_over_24_bytes", head(4, 24) + b"\x00" * 24, True)
    row(G, "array_count_25_over_24_bytes", head(4, 25) + b"\x00" * 24, False)
    row(G, "map_count_2_over_4_bytes", b"\xa2\x60\x00\x60\x00", True)
    row(G, "map_count_3_over_4_bytes", b"\xa3\x60\x00\x60\x00", False)
    row(G, "map_count_3_over_5_bytes", b"\xa3\x60\x00\x60\x00\x60", False)
    row(G, "map_with_an_odd_number_of_items_left", b"\xa2\x60\x00\x60", False)
    row(G, "map_of_1_without_its_value", b"\xa1\x61k", False)
    for major, what in ((4, "array"), (5, "map")):
        for n in (1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1):  # (2 · 2^63 is 0 in 64 bits)
            row(G, f"{what}_count_{n}", spell(major, n, 8) + b"\x60\x00", False)
        row(G, f"{what}_count_{(1 << 32) - 1}", spell(major, (1 << 32) - 1, 4) + b"\x60\x00", False)
    for depth in (1, 2, 8, 64, 200):
        row(G, f"nested_to_depth_{depth}", nested(depth, b"\x00"), True)
        row(G, f"nested_to_depth_{depth}_over_a_reserved_head", nested(depth, b"\x1c"), False)
        row(G, f"nested_to_depth_{depth}_over_bad_utf8", nested(depth, b"\x62\xc3\x28"), False)
    row(G, "array_of_every_major", array([uint(1), nint(-1), bstr(b"b"), text("t"), array([]), cmap([]), link(STD), NULL]), True)


_containers()


# ===== tags and links ===========================================================================================================
def identity_cid(n):
    """CIDv1, raw, identity hash over n bytes"""
    return b"\x01\x55\x00" + bytes([n]) + bytes(range(n))


def _tags():
    G = "tags"
    for t in list(range(42)) + [43]:
        row(G, f"tag_{t}", head(6, t) + bstr(b"\x00" + STD), False)
    for nb in (1, 2, 4, 8):
        row(G, f"tag_42_in_{nb}_bytes", spell(6, 42, nb) + bstr(b"\x00" + STD), True)
    row(G, "tag_42_over_a_text", b"\xd8\x2a" + text("bafy2bzace"), False)
    row(G, "tag_42_over_an_int", b"\xd8\x2a" + uint(5), False)
    row(G, "tag_42_over_an_empty_byte_string", b"\xd8\x2a" + bstr(b""), False)
    row(G, "tag_42_over_bytes_without_the_00", b"\xd8\x2a" + bstr(STD), False)
    row(G, "tag_42_over_only_the_00", b"\xd8\x2a" + bstr(b"\x00"), False)
    row(G, "tag_42_over_another_tag_42", b"\xd8\x2a" + link(STD), False)
    assert len(link(STD)) == 43
    row(G, "standard_43_byte_link", link(STD), True)
    row(G, "standard_link_string_head_59_00_27", b"\xd8\x2a\x59\x00\x27\x00" + STD, True)
    row(G, "standard_link_string_one_byte_longer", b"\xd8\x2a\x58\x28\x00" + STD + b"\x00", False)
    row(G, "standard_link_digest_one_byte_short", b"\xd8\x2a\x58\x26\x00" + STD[:-1], False)
    row(G, "cid_v0_link", link(V0), True)
    for n in (0, 1, 40, 41, 64, 65):
        row(G, f"identity_hash_link_digest_of_{n}", link(identity_cid(n)), n <= 64)


_tags()


# ===== CIDs inside a link =======================================================================================================
def varint(v):
    out = bytearray()
    while True:
        out.append((v & 0x7F) | (0x80 if v >> 7 else 0))
        v >>= 7
        if not v:
            return bytes(out)


def varint_padded(v):
    """the same value in one byte more: not minimal"""
    b = bytearray(varint(v))
    b[-1] |= 0x80
    return bytes(b) + b"\x00"


def cid(version=b"\x01", codec=b"\x71", code=b"\x12", size=None, digest=DIGEST):
    return version + codec + code + (varint(len(digest)) if size is None else size) + digest


VARINTS = {1: 0x71, 2: 0x80, 9: 1 << 56, 10: 1 << 63}  # a value whose minimal varint has that many bytes


def _cids():
    G = "cids"
    for v in (0, 1, 2):
        row(G, f"version_{v}", link(cid(version=varint(v))), v == 1)
    for nb, v in VARINTS.items():
        assert len(varint(v)) == nb
        row(G, f"codec_varint_of_{nb}_bytes", link(cid(codec=varint(v))), nb <= 9)  # unsigned-varint: nine bytes, 63 bits
        row(G, f"hash_code_varint_of_{nb}_bytes", link(cid(code=varint(v))), nb <= 9)
    row(G, "codec_varint_2_pow_63_minus_1", link(cid(codec=varint((1 << 63) - 1))), True)
    for field in ("version", "codec", "code", "size"):
        v = {"version": 1, "codec": 0x71, "code": 0x12, "size": 32}[field]
        row(G, f"{field}_varint_not_minimal", link(cid(**{field: varint_padded(v)})), False)
    row(G, "multihash_size_64", link(cid(digest=bytes(range(64)))), True)
    row(G, "multihash_size_65", link(cid(digest=bytes(range(65)))), False)
    row(G, "multihash_size_one_more_than_the_digest", link(cid(size=varint(33))), False)
    row(G, "multihash_size_one_less_than_the_digest", link(cid(size=varint(31))), False)
    row(G, "multihash_size_0_no_digest", link(cid(digest=b"")), True)
    row(G, "cid_cut_after_the_hash_code", link(b"\x01\x71\x12"), False)
    row(G, "cid_of_34_bytes_beginning_12_20", link(V0), True)
    row(G, "cid_of_35_bytes_beginning_12_20", link(V0 + b"\x00"), False)
    row(G, "cid_of_33_bytes_beginning_12_20", link(V0[:-1]), False)


_cids()

GROUPS = ("heads", "major7", "strings", "utf8", "containers", "tags", "cids")
assert tuple(dict.fromkeys(r.group for r in ROWS)) == GROUPS
BY_NAME = {r.name: r for r in ROWS}


# ===== the sweeps ===============================================================================================================
def table_cases(group):
    """every row of a group, row k of the table at block offset ≡ k (mod 16)"""
    return [Case(r.name, group, k % 16, r.item, r.ok) for k, r in enumerate(ROWS) if r.group == group]


def _residue_rows():
    names = [f"major0_arg_3_in_{nb}_bytes" for nb in (0, 1, 2, 4, 8)]                                    # one item per head width
    names += [f"major{m}_arg_{n}_in_8_bytes" for m in range(7) for n in (3, 42, 1 << 32, (1 << 64) - 1)]  # 8-byte arguments
    names += ["float64_one", "float64_all_ones"]
    names += [f"{what}_of_{n}" for what in ("bytes", "text") for n in (7, 8, 9, 15, 16, 17)]
    names += [f"{seq}_last_of_{total}" for seq in ("ed_a0_80", "ef_bf_bf", "f4_8f_bf_bf", "f4_90_80_80", "c3_cut_off") for total in (8, 9, 17)]
    names += ["standard_43_byte_link", "standard_link_string_head_59_00_27", "tag_42_in_2_bytes", "tag_42_in_4_bytes", "cid_v0_link"]
    names += [f"identity_hash_link_digest_of_{n}" for n in (0, 1, 40, 41, 64, 65)]
    return [BY_NAME[n] for n in names]


RESIDUE_ROWS = _residue_rows()
LINE_OFFSETS = tuple(range(112, 144))  # start offsets around the end of a block's first 128-byte line


def residue_cases():
    return [Case(f"{r.name}@{at}", "residues", at, r.item, r.ok) for r in RESIDUE_ROWS for at in tuple(range(16)) + LINE_OFFSETS]


BLOCK_END_MAX = 64


def block_end_cases(rows=None, group="block_end"):
    """every proper prefix of every well-formed item of at most 64 bytes as the last bytes of its block, and the item with
    one byte behind it; case k sits at block offset ≡ k (mod 16)"""
    out = []
    for r in (ROWS if rows is None else rows):
        if not r.ok or len(r.item) > BLOCK_END_MAX:
            continue
        for n in range(len(r.item)):
            out.append(Case(f"{r.name}[:{n}/{len(r.item)}]", group, len(out) % 16, r.item[:n], False))
        out.append(Case(f"{r.name}+00", group, len(out) % 16, r.item + b"\x00", False))
    return out


def cut_lengths(cases):
    """→ ({bytes kept}, {bytes cut off}) over the prefixes of a block-end sweep"""
    import re

    found = [re.search(r"\[:(\d+)/(\d+)\]$", c.name) for c in cases]
    return {int(m.group(1)) for m in found if m}, {int(m.group(2)) - int(m.group(1)) for m in found if m}


# the block-end cases that run once more as the LAST block of the arena: the items a fast path or a wide fetch looks ahead on
LAST_BLOCK_ROWS = ("standard_43_byte_link", "cid_v0_link", "identity_hash_link_digest_of_1", "major0_arg_18446744073709551615_in_8_bytes",
                   "float64_one", "text_of_9", "bytes_of_17", "ef_bf_bf_last_of_9")


LAST_BLOCK_TYPED = {"vec_u8": ("vec_of_9", "vec_of_32"), "cid": ("standard_43_byte_link",), "receipt": ("receipt_root_standard_link_return_data_of_3",),
                    "actor_state": ("actor_state_sequence_7",)}


def last_block_cases(kind="any"):
    """(name, at, item, ok) of the cases that run in a witness of their own, the carrier block last in the arena"""
    if kind == "any":
        rows = [BY_NAME[n] for n in LAST_BLOCK_ROWS]
        return [Case(r.name, "last_block", 0, r.item, True) for r in rows] + block_end_cases(rows, "last_block")
    return [c for c in typed_cases(kind) if c.name.split("[:")[0].split("+")[0] in LAST_BLOCK_TYPED[kind]]


# ===== typed values =============================================================================================================
def _vec_rows():
    """serde Vec<u8> of every length 0 … 40: every element in one byte, and ONE element spelled otherwise — first, at each
    position mod 8, and last → [Row]"""
    odd = {"18_80": (b"\x18\x80", True), "18_17_not_minimal": (b"\x18\x17", True), "19_00_80": (b"\x19\x00\x80", True),
           "18_ff": (b"\x18\xff", True), "19_01_00": (b"\x19\x01\x00", False)}
    out = []
    for n in range(41):
        plain = [bytes([(5 * i + n) % 24]) for i in range(n)]
        out.append(Row("vec_u8", f"vec_of_{n}", head(4, n) + b"".join(plain), True))
        if n:
            out.append(Row("vec_u8", f"vec_of_{n}_every_element_in_two_bytes", head(4, n) + b"".join(b"\x18" + bytes([0x18 + i]) for i in range(n)), True))
        for tag, (spelling, ok) in odd.items():
            for at in sorted(set(range(min(n, 8))) | ({n - 1} if n else set())):
                el = list(plain)
                el[at] = spelling
                out.append(Row("vec_u8", f"vec_of_{n}_element_{at}_spelled_{tag}", head(4, n) + b"".join(el), ok))
    out += [Row("vec_u8", "vec_head_98_05", b"\x98\x05" + bytes(5), True), Row("vec_u8", "vec_head_99_00_05", b"\x99\x00\x05" + bytes(5), True),
            Row("vec_u8", "vec_is_a_byte_string", bstr(b"\x01\x02"), False), Row("vec_u8", "vec_holds_a_negative", array([uint(1), nint(-1)]), False),
            Row("vec_u8", "vec_holds_a_text", array([text("1")]), False), Row("vec_u8", "vec_holds_null", array([NULL]), False),
            Row("vec_u8", "vec_element_255_in_8_bytes", array([uint(1), spell(0, 255, 8)]), True),
            Row("vec_u8", "vec_element_2_pow_32_in_8_bytes", array([uint(1), spell(0, 1 << 32, 8)]), False),
            Row("vec_u8", "vec_of_9_last_element_cut", head(4, 9) + bytes(8) + b"\x18", False),
            Row("vec_u8", "vec_count_one_more_than_its_elements", head(4, 9) + bytes(8), False)]
    return out


SHORT = b"\x01\x55\x00\x04name"  # CIDv1 raw, identity hash: the short form link_fast_len knows


def _receipt_rows():
    out = []
    roots = {"null": NULL, "standard_link": link(STD), "short_link": link(SHORT), "cid_v0_link": link(V0), "link_59_00_27": b"\xd8\x2a\x59\x00\x27\x00" + STD}
    for tag, root in roots.items():
        for n in range(18):  # (the return data is the padding: the events root moves through every residue)
            out.append(Row("receipt", f"receipt_root_{tag}_return_data_of_{n}", array([uint(0), bstr(bytes(range(n))), uint(1000 + n), root]), True))
    out += [Row("receipt", "receipt_root_is_a_uint", array([uint(0), bstr(b""), uint(1), uint(7)]), False),
            Row("receipt", "receipt_root_link_without_the_00", array([uint(0), bstr(b""), uint(1), b"\xd8\x2a" + bstr(STD)]), False),
            Row("receipt", "receipt_root_link_digest_one_byte_short", array([uint(0), bstr(b""), uint(1), b"\xd8\x2a\x58\x26\x00" + STD[:-1]]), False),
            Row("receipt", "receipt_exit_code_2_pow_32", array([uint(1 << 32), bstr(b""), uint(1), NULL]), False),
            Row("receipt", "receipt_exit_code_u32_max", array([uint((1 << 32) - 1), bstr(b""), uint(1), NULL]), True),
            Row("receipt", "receipt_gas_u64_max", array([uint(0), bstr(b""), uint((1 << 64) - 1), NULL]), True),
            Row("receipt", "receipt_gas_negative", array([uint(0), bstr(b""), nint(-1), NULL]), False),
            Row("receipt", "receipt_of_5", array([uint(0), bstr(b""), uint(1), NULL, NULL]), False),
            Row("receipt", "receipt_return_data_is_a_text", array([uint(0), text("r"), uint(1), NULL]), False)]
    return out


def _cid_rows():
    """every row of the tag and CID groups as a `cid` value (its verdict holds: each is a tag item), and three items that are
    well-formed and no link"""
    out = [Row("cid", r.name, r.item, r.ok) for r in ROWS if r.group in ("tags", "cids")]
    return out + [Row("cid", "cid_value_is_a_uint", uint(7), False), Row("cid", "cid_value_is_null", NULL, False),
                  Row("cid", "cid_value_is_the_cid_as_bytes", bstr(b"\x00" + STD), False)]


def actor_state(i=0, seq=None, bal=b"\x00\x05"):
    """fvm_shared ActorState in the spelling actor_entry_fast takes"""
    return array([link(pyamt.cid_of(b"code%d" % (i % 5))), link(pyamt.cid_of(b"state%d" % i)), uint(7) if seq is None else seq, bstr(bal), NULL])


TYPED_ROWS = {"vec_u8": _vec_rows(), "receipt": _receipt_rows(), "cid": _cid_rows()}
assert all(len({r.name for r in rows}) == len(rows) for rows in TYPED_ROWS.values())
KINDS = ("any", "vec_u8", "receipt", "cid", "actor_state")


def typed_cases(kind):
    """every row of a typed table at block offset ≡ its number (mod 16), then the block-end sweep of its well-formed rows"""
    if kind == "actor_state":  # the block-end variant only (the spellings: tests/hamt_get_cases.py)
        rows = [Row(kind, "actor_state_sequence_7", actor_state(1), True), Row(kind, "actor_state_sequence_2_pow_33", actor_state(2, uint(1 << 33)), True)]
        out = [Case(r.name, kind, k % 16, r.item, True) for k, r in enumerate(rows)]
        for r in rows:
            out += [Case(f"{r.name}[:{n}/{len(r.item)}]", kind, n % 16, r.item[:n], False) for n in range(len(r.item))]
            out.append(Case(f"{r.name}+00", kind, 0, r.item + b"\x00", False))
        return out
    rows = TYPED_ROWS[kind]
    out = [Case(r.name, kind, k % 16, r.item, r.ok) for k, r in enumerate(rows)]
    ends = [r for r in rows if r.ok and len(r.item) <= BLOCK_END_MAX]
    if kind == "vec_u8":
        ends = [r for r in ends if r.name in {f"vec_of_{n}" for n in (0, 1, 7, 8, 9, 16, 17, 32, 40)} | {"vec_of_12_every_element_in_two_bytes", "vec_of_9_element_8_spelled_18_ff"}]
    elif kind == "receipt":
        ends = [r for r in ends if r.name.endswith(("_return_data_of_0", "_return_data_of_3"))]
    else:
        ends = [r for r in ends if r.name in ("standard_43_byte_link", "cid_v0_link", "identity_hash_link_digest_of_1", "standard_link_string_head_59_00_27")]
    return out + block_end_cases(ends, kind)


ANY_GROUPS = GROUPS + ("residues", "block_end")  # what goes through the carriers with kind `any`
TYPED_KINDS = KINDS[1:]
_CASES = {}


def cases_of(group):
    """the cases of a table group, of a sweep ("residues", "block_end", "last_block") or of a typed kind"""
    if group not in _CASES:
        _CASES[group] = (residue_cases() if group == "residues" else block_end_cases() if group == "block_end" else last_block_cases()
                         if group == "last_block" else typed_cases(group) if group in TYPED_KINDS else table_cases(group))
    return _CASES[group]


def kind_of(group):
    return group if group in TYPED_KINDS else "any"


# ===== carriers =================================================================================================================
Batch =collections.namedtuple("Batch", "store root queries want values blocks offsets cids")
#   queries   AMT indices / HAMT keys, one per case;  want  the status of each;  values  the item's bytes where want is TRUE
#   blocks    the carrier block of each case;  offsets  where its item begins in it;  cids  the carrier blocks' CIDs


def pad_len(c0, at):
    """the length p of a pad string such that an item behind `c0` bytes and the string `head ‖ p bytes` begins at block offset
    ≡ at (mod 16) for at < 16, or at offset `at`"""
    if at < 16:
        return next(p for p in range(40) if (c0 + len(head(2, p)) + p) % 16 == at)
    for hl in (1, 2, 3, 5):
        p = at - c0 - hl
        if p >= 0 and len(head(2, p)) == hl:
            return p
    raise AssertionError((c0, at))  # (offset c0 + 25 has no pad: a string of 23 takes 24 bytes, one of 24 takes 26)


def chunks(n):
    """128-byte lines a block of n bytes takes in the arena"""
    return max(1, (n + 127) // 128)


AMT_SHAPE = {0: (3, 512), 3: (5, 1024)}  # version → (bit width, cases per tree: one leaf each, the tree two or three levels over them)
PADDED = ("any", "vec_u8")               # kinds whose AMT leaf holds a pad value in front of the item


def amt_batch(cases, version, kind="any", last_block=False) -> Batch:
    """one leaf `[bitmap, [], [pad, item]]` per case under one root (typed kinds without a pad value: `[item]`)"""
    bw, per_tree = AMT_SHAPE[version]
    assert 0 < len(cases) <= per_tree
    width = 1 << bw
    c0 = 1 + len(bstr(bytes((width + 7) // 8))) + 1 + 1
    items, queries, offsets = {}, [], []
    for L, c in enumerate(cases):
        base = L * width
        if kind in PADDED:
            p = pad_len(c0, c.at)
            items[base] = head(4 if kind == "vec_u8" else 2, p) + bytes(p)
            items[base + 1] = c.item
            offsets.append(c0 + len(items[base]))
        else:
            items[base] = c.item
            offsets.append(c0)
        queries.append(base + (kind in PADDED))
    top, height = max(items), 0
    while top >= width ** (height + 1):
        height += 1
    st, where = pyamt.Store(), {}
    root = pyamt.build_amt(st, items, version=version, bit_width=bw, height=max(height, 1), where=where)
    cids = [where[(0, L * width)] for L in range(len(cases))]
    if last_block:
        assert len(cases) == 1
        st.blocks[cids[0]] = st.blocks.pop(cids[0])
        assert list(st.blocks)[-1] == cids[0] and chunks(len(st.blocks[cids[0]])) == min(chunks(len(b)) for b in st.blocks.values()) == 1
    blocks = [st.blocks[c] for c in cids]
    for c, b, o in zip(cases, blocks, offsets):
        assert b[o:] == c.item and (kind not in PADDED or (o % 16 == c.at if c.at < 16 else o == c.at)), c.name  # the residues come out as intended
    return Batch(st, root, queries, [TRUE if c.ok else DECODE for c in cases], [c.item if c.ok else None for c in cases], blocks, offsets, cids)


_HAMT_KEYS = []


def hamt_keys():
    """1024 keys of 32 bytes, key s on the path (s >> 5, s & 31) of a width-5 tree"""
    if not _HAMT_KEYS:
        have, n = {}, 0
        while len(have) < 1024:
            k = hashlib.sha256(b"cbor item key %d" % n).digest()
            n += 1
            have.setdefault((pyhamt.index_at(k, 0, 5) << 5) | pyhamt.index_at(k, 1, 5), k)
        _HAMT_KEYS.extend(have[s] for s in range(1024))
    return _HAMT_KEYS


FILLER = {"any": uint(0), "vec_u8": b"\x80", "cid": link(STD), "receipt": pyamt.receipt(), "actor_state": actor_state()}
HAMT_PER_TREE = 1024


def hamt_leaf(key, kind, at, item, depth=2):
    """`[bitfield, [[[pad key, filler], [key, item]]]]` → (block, offset of the item)"""
    bf = 1 << pyhamt.index_at(key, depth, 5)
    front = head(4, 2) + bstr(bf.to_bytes((bf.bit_length() + 7) // 8, "big")) + head(4, 1) + head(4, 2) + head(4, 2)
    back = FILLER[kind] + head(4, 2) + bstr(key)
    p = pad_len(len(front) + len(back), at)
    front += bstr(bytes(p)) + back
    return front + item, len(front)


def _links_node(children):
    bf = 0
    for j in children:
        bf |= 1 << j
    return array([bstr(bf.to_bytes((bf.bit_length() + 7) // 8, "big")), array([link(children[j]) for j in sorted(children)])])


def hamt_batch(cases, kind="any", last_block=False) -> Batch:
    """one leaf node per case, at the end of its key's path through a root and a middle node of links"""
    assert 0 < len(cases) <= HAMT_PER_TREE
    keys = hamt_keys()[: len(cases)]
    st = pyamt.Store()
    blocks, offsets, cids, mids = [], [], [], {}
    for s, c in enumerate(cases):
        b, o = hamt_leaf(keys[s], kind, c.at, c.item)
        assert b[o:] == c.item and (o % 16 == c.at if c.at < 16 else o == c.at), c.name  # the residues come out as intended
        blocks.append(b)
        offsets.append(o)
        cids.append(st.put(b))
        mids.setdefault(s >> 5, {})[s & 31] = cids[-1]
    if last_block:  # the two link nodes hold 32 links (31 of them to blocks no witness holds): they are LONGER than the leaf
        assert len(cases) == 1
        absent = {j: pyamt.cid_of(b"no such node %d" % j) for j in range(32)}
        mids = {i: {**absent, **ch} for i, ch in mids.items()}
        root = st.put(_links_node({**absent, **{i: st.put(_links_node(ch)) for i, ch in mids.items()}}))
        st.blocks[cids[0]] = st.blocks.pop(cids[0])
        assert list(st.blocks)[-1] == cids[0] and chunks(len(blocks[0])) == min(chunks(len(b)) for b in st.blocks.values())
        assert sum(chunks(len(b)) == chunks(len(blocks[0])) for b in st.blocks.values()) == 1
    else:
        root = st.put(_links_node({i: st.put(_links_node(ch)) for i, ch in mids.items()}))
    return Batch(st, root, keys, [TRUE if c.ok else DECODE for c in cases], [c.item if c.ok else None for c in cases], blocks, offsets, cids)


def batches(cases, per):
    return [cases[i: i + per] for i in range(0, len(cases), per)]



# ---- headers -------------------------------------------------------------------------------------------------------------------
# The part of the table that goes into a block header, and why: a header case costs a block of its own and a claim of its
# own, so the rows are the ones on which the LDS reader differs from the window reader — its second head() (one item per head
# width, every 8-byte argument of the residue subset, every reserved additional info, every major-7 row), its second text_ok
# (every UTF-8 sequence alone, in a text of 8 and as the last bytes of a text of 9 and 17) and every link form — and the block-end
# prefixes of the LAST_BLOCK rows in field 15, whose end is the end of the header.
def _header_rows():
    rows = list(RESIDUE_ROWS)
    rows += [r for r in ROWS if r.group == "major7" or "additional_info" in r.name]
    rows += [r for r in ROWS if r.group == "utf8" and r.name.endswith(("_alone", "_last_of_8", "_last_of_9", "_last_of_17"))]
    rows += [r for r in ROWS if r.group == "cids" or (r.group == "tags" and (not r.name.startswith("tag_") or r.name.startswith("tag_42")))]
    return list({r.name: r for r in rows}.values())


HEADER_ROWS = _header_rows()
HEADER_STAGE = 8192   # the tipset prologue stages a header of up to 8 KB in LDS (tipset_prepare.hip)
HEADER_ARRAY_HEADS = {1: b"\x90", 2: b"\x98\x10", 3: b"\x99\x00\x10", 5: b"\x9a\x00\x00\x00\x10", 9: b"\x9b" + (16).to_bytes(8, "big")}


def header_cases():
    """→ [(name, field, at, item, the item is well-formed)]: field 0 behind each spelling of the tuple's head (offsets 1, 2, 3, 5,
    9), field 15 at residue k mod 16 behind a pad in field 13 — short, and long enough to lift the header over the stage"""
    out = []
    for k, r in enumerate(HEADER_ROWS):
        out.append((f"{r.name}/field0", 0, sorted(HEADER_ARRAY_HEADS)[k % 5], r.item, r.ok))
        out.append((f"{r.name}/field15", 15, k % 16, r.item, r.ok))
        out.append((f"{r.name}/field15_long_header", 15, HEADER_STAGE + 16 + k % 16, r.item, r.ok))
    for c in block_end_cases([BY_NAME[n] for n in LAST_BLOCK_ROWS]):
        out.append((f"{c.name}/field15", 15, c.at, c.item, False))
    return out


def header_respell(field, at, item):
    """header override for storage_chain_cases.chain / event_chain_cases.tipset: the 16 default fields → the header's bytes
    with `item` as field 0 or 15 at the block offset asked for"""
    def make(f):
        if field == 0:
            return HEADER_ARRAY_HEADS[at] + item + b"".join(f[1:])
        before = b"\x90" + b"".join(f[:13])
        p = pad_len(len(before) + len(f[14]), at)
        b = before + bstr(bytes(p)) + f[14]
        assert len(b) % 16 == at if at < 16 else len(b) == at
        return b + item
    return make


@functools.lru_cache(maxsize=None)
def header_chains(which, long_headers):
    """every header case as the child header of a chain of its own, all chains in ONE witness (the blocks under the header are
    the same for every case) → (store, [claim], [case name], [the item is well-formed]).  which: "storage" | "events".  The
    cases whose header is longer than the prologue's stage go into a witness of their own (`long_headers`): the event
    verifier picks its header reader by the longest block of the witness."""
    import event_chain_cases as ec
    import storage_chain_cases as sc

    st, claims, names, oks = pyamt.Store(), [], [], []
    for name, field, at, item, ok in header_cases():
        if (at > HEADER_STAGE) != long_headers:
            continue
        respell = header_respell(field, at, item)
        if which == "storage":
            one, claim, _ = sc.chain(sc.layout("C", sc.PAIRS), sc.S[2], sc.VAL[2], salt=5, header=respell)
        else:
            one, claim, _ = ec.tipset(salt=5, child_header=respell)
        for c, b in one.blocks.items():
            assert st.blocks.setdefault(c, b) == b, name
        claims.append(claim)
        names.append(name)
        oks.append(ok)
    assert (max(len(b) for b in st.blocks.values()) > HEADER_STAGE) == long_headers
    return st, claims, names, oks
