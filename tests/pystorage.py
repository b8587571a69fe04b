"""A plain, slow restatement of `verify_storage_proof` (src/proofs/storage/verifier.rs:24-63) in Python: the second
judge of the storage chain next to the C++ oracle.  Written from the reference's Rust (storage/verifier.rs,
storage/decode.rs, common/decode.rs, common/evm.rs, trust/mod.rs) and SURVEY.md A.1, A.4, A.6, A.8-A.10.

    verify(blocks: {cid bytes: block bytes}, claim: dict, trust=None) -> status byte (include/ipcfp.h)

`claim` holds the fields of `StorageProof` as the reference's struct does (strings stay strings): child_epoch,
child_block_cid, parent_state_root, actor_id, actor_state_cid, storage_root, slot, value.  `trust` is None (AcceptAll)
or (ec_chain_empty, min_epoch, max_epoch) (F3Certificate, cert.rs:52-64).

It works on TREES: a block is decoded whole into Python values by a strict DAG-CBOR reader and the typed decodes
(`HeaderLite`, `StateRoot`, `ActorState`, `EvmStateV6/V5`, the six storage-root layouts, HAMT nodes) are shape checks
on the tree — serde's streaming order never matters, because a failed decode is one outcome whatever failed first.

HOW FAR IT IS INDEPENDENT.  Everything the reference's own text decides — the order of the verifier's steps, the
six-way sniff and its fall-through rules, `bw as u32`, left_pad_32, the string compares, that `load_with_bit_width` is
called (and so fetches the root) before anything looks at the width — is read here from the Rust alone, and a
disagreement with the oracle or the engine on such a point is a finding.  What fvm_ipld_hamt and serde do INSIDE is not
in the reference's text and their sources are not at hand: there this file follows SURVEY.md A.6, and where A.6 is
silent it makes the SAME choice the oracle and the engine were written to make.  Those choices have NAMES (the
constants below); on them the three judges are one judge, and tests/assumption_cases.py STORAGE_CASES holds a case per
name, so that each is confirmed or flipped in one place the day the crates can be read.  Three of the four go against
what a reader of A.6's format line ("bucket, ≤ 3, sorted by key") or of a popcount check at decode would expect: an
over-full or unsorted bucket is searched, and `[h'01', []]` is an error only for a key that lands on bit 0."""
import base64
import hashlib

FALSE_UNTRUSTED_CHILD, FALSE_STATE_ROOT, FALSE_ACTOR_STATE, FALSE_STORAGE_ROOT, FALSE_VALUE = 3, 18, 19, 20, 21
TRUE, ERR_MISSING_BLOCK, ERR_DECODE, ERR_ACTOR_NOT_FOUND, ERR_BAD_CLAIM, ERR_MAX_DEPTH = 1, 65, 66, 68, 69, 70

# ---- the named assumptions about serde / serde_ipld_dagcbor / fvm_ipld_hamt -------------------------------------
# (what the oracle and the engine were written to do as well: tests/assumption_cases.py STORAGE_CASES, one case each)
# a serde-derived struct (SmallMap, MapStruct) is read from a CBOR MAP only; the same fields offered as an array are
# a decode error of that attempt (serde's derive has a visit_seq, the DAG-CBOR deserializer never calls it)
STRUCT_FROM_ARRAY_IS_REJECTED = True
# popcount(bitfield) is compared with the pointer list only where a get INDEXES the list, not when the node is
# decoded: a node whose bitfield names more pointers than it has is an Err for the keys that land on a missing
# pointer, and is walked like any other node by the rest
HAMT_POINTER_COUNT_IS_CHECKED_WHEN_INDEXED = True
# a bucket is searched as it stands: more than 3 pairs, or pairs out of order, are a writer's business
HAMT_BUCKET_SIZE_AND_ORDER_ARE_NOT_CHECKED_ON_READ = True
# `load_with_bit_width` takes any u32 and does not look at it; `HashBits::next` refuses a width of 0 or of more than 8,
# which makes it an Err of the GET, reported like a malformed node — after the root block was fetched and decoded
HAMT_BIT_WIDTH_OUTSIDE_1_TO_8_IS_AN_ERR_OF_THE_GET = True


class Err(Exception):
    def __init__(self, status, what=""):
        super().__init__(what)
        self.status = status


class Link:
    __slots__ = ("cid",)

    def __init__(self, cid):
        self.cid = cid


class Map:
    """A CBOR map as the list of its (key, value) entries, in order, duplicates kept."""
    __slots__ = ("entries",)

    def __init__(self, entries):
        self.entries = entries


# ---- CIDs -----------------------------------------------------------------------------------------
def _varint(b, pos):
    """Unsigned LEB128, minimal, at most 9 bytes (unsigned-varint) → (value, next pos)."""
    v = shift = 0
    for k in range(9):
        if pos >= len(b):
            raise ValueError("varint cut short")
        x = b[pos]
        pos += 1
        v |= (x & 0x7F) << shift
        shift += 7
        if not x & 0x80:
            if x == 0 and k > 0:
                raise ValueError("varint not minimal")
            return v, pos
    raise ValueError("varint too long")


def check_cid(b: bytes) -> bytes:
    """The bytes are exactly one CID (v0: a bare sha2-256 multihash; v1: version, codec, multihash of ≤ 64 bytes)."""
    if len(b) == 34 and b[0] == 0x12 and b[1] == 0x20:
        return b
    ver, pos = _varint(b, 0)
    if ver != 1:
        raise ValueError("CID version")
    _codec, pos = _varint(b, pos)
    _code, pos = _varint(b, pos)
    size, pos = _varint(b, pos)
    if size > 64 or len(b) - pos != size:
        raise ValueError("multihash length")
    return b


_B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def _b58decode(s):
    n = 0
    for ch in s:
        n = n * 58 + _B58.index(ch)  # ValueError on a foreign character
    body = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return b"\0" * (len(s) - len(s.lstrip("1"))) + body


def _b58encode(b):
    n = int.from_bytes(b, "big")
    out = ""
    while n:
        n, r = divmod(n, 58)
        out = _B58[r] + out
    return "1" * (len(b) - len(b.lstrip(b"\0"))) + out


def _b32decode(s, alphabet):
    bits = n = 0
    out = bytearray()
    for ch in s:
        bits = (bits << 5) | alphabet.index(ch)
        n += 5
        if n >= 8:
            n -= 8
            out.append((bits >> n) & 0xFF)
    if n >= 5 or bits & ((1 << n) - 1):
        raise ValueError("base32 tail")
    return bytes(out)


def cid_from_string(s: str) -> bytes:
    """`Cid::try_from(&str)`: ValueError where the reference's parse_cid is Err (common/witness.rs:60-63)."""
    at = s.find("/ipfs/")
    if at >= 0:
        s = s[at + 6:]
    if len(s) == 46 and s.startswith("Qm"):
        return check_cid(_b58decode(s))
    if len(s) < 2:
        raise ValueError("too short")
    base, body = s[0], s[1:]
    if base == "b":
        raw = _b32decode(body, "abcdefghijklmnopqrstuvwxyz234567")
    elif base == "B":
        raw = _b32decode(body, "ABCDEFGHIJKLMNOPQRSTUVWXYZ234567")
    elif base in "fF":
        digits = "0123456789abcdef" if base == "f" else "0123456789ABCDEF"
        if len(body) % 2 or any(ch not in digits for ch in body):
            raise ValueError("base16")
        raw = bytes.fromhex(body)
    elif base == "z":
        raw = _b58decode(body)
    else:
        raise ValueError("multibase")  # (the other alphabets: include/ipcfp.h names them an engine limit)
    return check_cid(raw)


def cid_to_string(cid: bytes) -> str:
    """`Cid::to_string()`: base58btc for a CIDv0, "b" + base32-lower without padding for a CIDv1."""
    if len(cid) == 34 and cid[0] == 0x12:
        return _b58encode(cid)
    return "b" + base64.b32encode(cid).decode().lower().rstrip("=")


# ---- the strict DAG-CBOR reader (the rules tests/assumption_cases.py names) -------------------------
def _item(b, pos):
    if pos >= len(b):
        raise Err(ERR_DECODE, "item cut short")
    major, info = b[pos] >> 5, b[pos] & 31
    pos += 1
    if major == 7:
        if info == 20:
            return False, pos
        if info == 21:
            return True, pos
        if info == 22:
            return None, pos
        if info == 27:
            if pos + 8 > len(b):
                raise Err(ERR_DECODE, "float cut short")
            return float(int.from_bytes(b[pos:pos + 8], "big")), pos + 8  # (only its being a float matters here)
        raise Err(ERR_DECODE, "simple value / short float / break")
    if info < 24:
        arg = info
    elif info <= 27:
        nb = 1 << (info - 24)
        if pos + nb > len(b):
            raise Err(ERR_DECODE, "head cut short")
        arg = int.from_bytes(b[pos:pos + nb], "big")  # a non-minimal head is accepted
        pos += nb
    else:
        raise Err(ERR_DECODE, "indefinite length or reserved head")
    if major == 0:
        return arg, pos
    if major == 1:
        return -1 - arg, pos
    if major in (2, 3):
        if pos + arg > len(b):
            raise Err(ERR_DECODE, "string cut short")
        raw = bytes(b[pos:pos + arg])
        if major == 2:
            return raw, pos + arg
        try:
            return raw.decode("utf-8"), pos + arg
        except UnicodeDecodeError:
            raise Err(ERR_DECODE, "text is not UTF-8")
    if major == 4:
        out = []
        for _ in range(arg):
            v, pos = _item(b, pos)
            out.append(v)
        return out, pos
    if major == 5:
        ents = []
        for _ in range(arg):
            k, pos = _item(b, pos)
            v, pos = _item(b, pos)
            ents.append((k, v))
        return Map(ents), pos
    if arg != 42:
        raise Err(ERR_DECODE, "a tag other than 42")
    inner, pos = _item(b, pos)
    if type(inner) is not bytes or inner[:1] != b"\0":
        raise Err(ERR_DECODE, "link without the identity multibase prefix")
    try:
        return Link(check_cid(inner[1:])), pos
    except ValueError as e:
        raise Err(ERR_DECODE, f"link: {e}")


def decode(block: bytes):
    """One block → one tree; trailing bytes are a decode error."""
    v, pos = _item(block, 0)
    if pos != len(block):
        raise Err(ERR_DECODE, "trailing bytes")
    return v


def _bad(what):
    raise Err(ERR_DECODE, what)


def _tuple(x, n, what):
    if type(x) is not list or len(x) != n:
        _bad(f"{what}: not an array of {n}")
    return x


def _cid(x, what):
    if type(x) is not Link:
        _bad(f"{what}: not a link")
    return x.cid


def _u64(x, what):
    if type(x) is not int or not 0 <= x < 1 << 64:
        _bad(f"{what}: not a u64")
    return x


def _i64(x, what):
    if type(x) is not int or not -(1 << 63) <= x < 1 << 63:
        _bad(f"{what}: not an i64")
    return x


def _bytes(x, what):
    if type(x) is not bytes:
        _bad(f"{what}: not a byte string")
    return x


# ---- typed decodes (common/decode.rs) ----------------------------------------------------------------
def header_parent_state_root(block):
    """`extract_parent_state_root`: HeaderLite, a 16-tuple (common/decode.rs:100-124)."""
    h = _tuple(decode(block), 16, "header")
    if type(h[5]) is not list:
        _bad("parents")
    for p in h[5]:
        _cid(p, "parent")
    _i64(h[7], "height")
    for k in (8, 9, 10):
        _cid(h[k], f"header field {k}")
    _u64(h[12], "timestamp")
    _u64(h[14], "fork_signaling")
    return h[8].cid


def state_root_actors(block):
    """fvm_shared `StateRoot` [version, actors, info]; StateTreeVersion knows 0..5."""
    s = _tuple(decode(block), 3, "StateRoot")
    if _u64(s[0], "version") > 5:
        _bad("StateTreeVersion")
    _cid(s[2], "info")
    return _cid(s[1], "actors")


def _check_address(b):
    if not b:
        _bad("empty address")
    proto, body = b[0], b[1:]
    try:
        if proto == 0:
            v, pos = _varint(body, 0)
            ok = pos == len(body)
        elif proto in (1, 2):
            ok = len(body) == 20
        elif proto == 3:
            ok = len(body) == 48
        elif proto == 4:
            _ns, pos = _varint(body, 0)
            ok = len(body) - pos <= 54
        else:
            ok = False
    except ValueError:
        ok = False
    if not ok:
        _bad("address")


def check_actor_state(x):
    """fvm_shared `ActorState` [code, state, sequence, balance, delegated_address] → the tree itself."""
    a = _tuple(x, 5, "ActorState")
    _cid(a[0], "code")
    _cid(a[1], "state")
    _u64(a[2], "sequence")
    bal = _bytes(a[3], "balance")  # BigInt bytes: empty for zero, else a sign byte 00 / 01 and the magnitude
    if len(bal) > 128:
        _bad("balance of more than 128 bytes")  # (fvm_shared's BigInt reader refuses a longer one)
    if bal and bal[0] > 1:
        _bad("balance sign")
    if a[4] is not None:
        _check_address(_bytes(a[4], "delegated_address"))
    return a


def check_vec_u8(x):
    """serde `Vec<u8>`: an array of integers 0..255 → bytes."""
    if type(x) is not list or any(type(e) is not int or not 0 <= e <= 255 for e in x):
        _bad("Vec<u8>")
    return bytes(x)


def evm_contract_state(block):
    """`parse_evm_state` (common/decode.rs:79-97): the 6-tuple first, then the 5-tuple."""
    e = decode(block)

    def common(t):
        _cid(t[0], "bytecode")
        if len(_bytes(t[1], "bytecode_hash")) != 32:
            _bad("bytecode_hash is not 32 bytes")
        return _cid(t[2], "contract_state")

    try:
        t = _tuple(e, 6, "EvmStateV6")
        root = common(t)
        _u64(t[4], "nonce")  # [3] and [5]: Option<IgnoredAny> — null or anything
        return root
    except Err:
        pass
    t = _tuple(e, 5, "EvmStateV5")
    root = common(t)
    _u64(t[3], "nonce")
    return root


# ---- HAMT --------------------------------------------------------------------------------------------
class _HashBits:
    """`HashBits` over SHA-256(key): `next(n)` hands out the next n bits, most significant first."""

    def __init__(self, key):
        self.digest = int.from_bytes(hashlib.sha256(key).digest(), "big")
        self.used = 0

    def next(self, n):
        if not 1 <= n <= 8:
            raise Err(ERR_DECODE, "HashBits::next: bit length")  # HAMT_BIT_WIDTH_OUTSIDE_1_TO_8_IS_AN_ERR_OF_THE_GET
        if self.used + n > 256:
            raise Err(ERR_MAX_DEPTH, "HashBits::next: no bits left")
        self.used += n
        return (self.digest >> (256 - self.used)) & ((1 << n) - 1)


def _load_node(blocks, cid, check_value):
    """`store.get_cbor::<Node>(cid)`: absent → Err; else the block decoded as ONE serde value
    `(bitfield bytes, [pointer…])`, every pointer a link or a list of (key bytes, V) pairs — a wrong type anywhere in
    the block, also in a bucket the key never visits, fails the node.  → (bitfield int, pointers)"""
    if cid not in blocks:
        raise Err(ERR_MISSING_BLOCK, "HAMT node")
    bf, plist = _tuple(decode(blocks[cid]), 2, "HAMT node")
    if len(_bytes(bf, "bitfield")) > 32:
        _bad("bitfield of more than 256 bits")
    if type(plist) is not list:
        _bad("pointers")
    pointers = []
    for p in plist:
        if type(p) is list:
            p = [(_bytes(_tuple(kv, 2, "pair")[0], "key"), check_value(kv[1])) for kv in p]
        elif type(p) is not Link:
            _bad("pointer")
        pointers.append(p)
    return int.from_bytes(bf, "big"), pointers


def _hamt_find(blocks, root, bit_width, key, check_value):
    """The walk of `Hamt::load_with_bit_width(root, store, bw)?.get(key)?` → (node block, pointer number, pair number,
    checked value) of the pair that holds the key, or None.
    load reads the root block and nothing else — it does not look at the width (decode.rs:79-80: a missing root is the
    `?` of the load, whatever the width); get hashes the key and walks: at each node `HashBits::next(bw)`, bit clear ⇒
    None, else child number popcount(bits below); a link ⇒ load that node and go on; a bucket ⇒ linear search."""
    at = root
    bitfield, pointers = _load_node(blocks, at, check_value)
    bits = _HashBits(key)
    while True:
        idx = bits.next(bit_width)
        if not (bitfield >> idx) & 1:
            return None
        below = bin(bitfield & ((1 << idx) - 1)).count("1")
        if below >= len(pointers):
            _bad("child index past the pointer list")  # HAMT_POINTER_COUNT_IS_CHECKED_WHEN_INDEXED
        child = pointers[below]
        if type(child) is Link:
            at = child.cid
            bitfield, pointers = _load_node(blocks, at, check_value)
            continue
        for n, (k, v) in enumerate(child):  # HAMT_BUCKET_SIZE_AND_ORDER_ARE_NOT_CHECKED_ON_READ
            if k == key:
                return blocks[at], below, n, v
        return None


def hamt_get(blocks, root, bit_width, key, check_value):
    """→ the checked value, or None"""
    found = _hamt_find(blocks, root, bit_width, key, check_value)
    return None if found is None else found[3]


def _head(b, pos):
    """the head of an item that is known to decode → (argument, position behind the head)"""
    info = b[pos] & 31
    if info < 24:
        return info, pos + 1
    nb = 1 << (info - 24)
    return int.from_bytes(b[pos + 1:pos + 1 + nb], "big"), pos + 1 + nb


def hamt_get_bytes(blocks, root, bit_width, key, check_value):
    """`hamt_get`, answering with the value's own bytes as the node spells them (what the primitive ipcfp_hamt_get
    LOCATES; the storage chain only ever needed the decoded value) → bytes, or None."""
    found = _hamt_find(blocks, root, bit_width, key, check_value)
    if found is None:
        return None
    b, pointer, pair, _ = found
    _, pos = _head(b, 0)                 # [bitfield, pointers]
    _, pos = _item(b, pos)
    _, pos = _head(b, pos)
    for _ in range(pointer):
        _, pos = _item(b, pos)
    _, pos = _head(b, pos)               # the bucket
    for _ in range(pair):
        _, pos = _item(b, pos)
    _, pos = _head(b, pos)               # [key, value]
    _, pos = _item(b, pos)
    _, end = _item(b, pos)
    return bytes(b[pos:end])


# ---- read_storage_slot (storage/decode.rs:36-97) -----------------------------------------------------------------------
def _small_map(x):
    """`SmallMap { v: Vec<(ByteBuf, ByteBuf)> }` → the pairs; unknown fields are skipped, a second "v" is an error."""
    if type(x) is not Map:
        _bad("SmallMap is not a map")  # STRUCT_FROM_ARRAY_IS_REJECTED
    pairs = None
    for k, v in x.entries:
        if type(k) is not str:
            _bad("field name")
        if k == "v":
            if pairs is not None:
                _bad("duplicate field v")
            if type(v) is not list:
                _bad("v")
            pairs = [(_bytes(_tuple(p, 2, "pair")[0], "key"), _bytes(p[1], "value")) for p in v]
    if pairs is None:
        _bad("missing field v")
    return pairs


def _first(pairs, slot):
    for k, v in pairs:
        if k == slot:
            return v
    return None


def read_storage_slot(blocks, root, slot):
    if root not in blocks:
        raise Err(ERR_MISSING_BLOCK, "contract_state root")
    raw = blocks[root]

    def attempt(fn):
        try:
            return True, fn(decode(raw))
        except Err:
            return False, None

    # A1) [params bytes, [SmallMap…]] — every map must decode, the first is searched, an empty list falls through
    ok, maps = attempt(lambda t: (_bytes(_tuple(t, 2, "A1")[0], "params"),
                                  [_small_map(m) for m in (t[1] if type(t[1]) is list else _bad("list"))])[1])
    if ok and maps:
        return _first(maps[0], slot)
    # A2) [params bytes, SmallMap]
    ok, pairs = attempt(lambda t: (_bytes(_tuple(t, 2, "A2")[0], "params"), _small_map(t[1]))[1])
    if ok:
        return _first(pairs, slot)
    # A3) SmallMap
    ok, pairs = attempt(_small_map)
    if ok:
        return _first(pairs, slot)
    # B1) [root cid, bitwidth u64]   B2) { root, bitwidth, .. }   C) the block itself is a node, width 5
    hroot, bw = root, 5
    ok, got = attempt(lambda t: (_cid(_tuple(t, 2, "B1")[0], "root"), _u64(t[1], "bitwidth")))
    if not ok:
        def map_struct(t):
            if type(t) is not Map:
                _bad("MapStruct is not a map")
            seen = {}
            for k, v in t.entries:
                if type(k) is not str:
                    _bad("field name")
                if k in ("root", "bitwidth"):
                    if k in seen:
                        _bad("duplicate field")
                    seen[k] = _cid(v, k) if k == "root" else _u64(v, k)
            if len(seen) != 2:
                _bad("missing field")
            return seen["root"], seen["bitwidth"]
        ok, got = attempt(map_struct)
    if ok:
        hroot, bw = got[0], got[1] & 0xFFFFFFFF  # `bw as u32`
    return hamt_get(blocks, hroot, bw, slot, check_vec_u8)


def left_pad_32(v: bytes) -> bytes:
    return v[-32:] if len(v) >= 32 else bytes(32 - len(v)) + v


# ---- verify_storage_proof ---------------------------------------------------------------------------------------------
def _parse_cid(s):
    try:
        return cid_from_string(s)
    except ValueError:
        raise Err(ERR_BAD_CLAIM, "unparsable CID string")


def _verify(blocks, c, trust):
    child = _parse_cid(c["child_block_cid"])                                  # verifier.rs:85
    if trust is not None:
        empty, lo, hi = trust
        if empty or not lo <= c["child_epoch"] <= hi:
            return FALSE_UNTRUSTED_CHILD                                      # :87
    _parse_cid(c["child_block_cid"])                                          # :38
    if child not in blocks:
        raise Err(ERR_MISSING_BLOCK, "child header")                          # :101-103
    if cid_to_string(header_parent_state_root(blocks[child])) != c["parent_state_root"]:
        return FALSE_STATE_ROOT                                               # :110
    sroot = _parse_cid(c["parent_state_root"])                                # :44
    if sroot not in blocks:
        raise Err(ERR_MISSING_BLOCK, "StateRoot")                             # common/decode.rs:23-25
    actors = state_root_actors(blocks[sroot])
    n, key = c["actor_id"], bytearray(b"\0")
    while True:                                                               # Address::new_id(n).to_bytes()
        key.append((n & 0x7F) | (0x80 if n >> 7 else 0))
        n >>= 7
        if not n:
            break
    actor = hamt_get(blocks, actors, 5, bytes(key), check_actor_state)
    if actor is None:
        raise Err(ERR_ACTOR_NOT_FOUND, "actor not found")                     # common/decode.rs:39
    if cid_to_string(actor[1].cid) != c["actor_state_cid"]:
        return FALSE_ACTOR_STATE                                              # :126
    astate = _parse_cid(c["actor_state_cid"])                                 # :55
    if astate not in blocks:
        raise Err(ERR_MISSING_BLOCK, "EVM state")                             # :136-138
    if cid_to_string(evm_contract_state(blocks[astate])) != c["storage_root"]:
        return FALSE_STORAGE_ROOT                                             # :144
    root = _parse_cid(c["storage_root"])                                      # :61
    s = c["slot"]
    while s.startswith("0x"):                                                 # trim_start_matches("0x")
        s = s[2:]
    if len(s) != 64 or any(ch not in "0123456789abcdefABCDEF" for ch in s):
        raise Err(ERR_BAD_CLAIM, "slot hex")                                  # :155-157
    value = read_storage_slot(blocks, root, bytes.fromhex(s)) or b""          # :160-162
    actual = "0x" + left_pad_32(value).hex()
    return TRUE if actual.lower() == _ascii_lower(c["value"]) else FALSE_VALUE  # eq_ignore_ascii_case, :169


def _ascii_lower(s):
    return "".join(chr(ord(ch) + 32) if "A" <= ch <= "Z" else ch for ch in s)


def verify(blocks, claim, trust=None) -> int:
    try:
        return _verify(blocks, claim, trust)
    except Err as e:
        return e.status
