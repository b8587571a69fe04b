"""A plain restatement of `generate_storage_proof` steps 1-4 (src/proofs/storage/generator.rs:72-155) in Python, over
tests/pystorage.py's decodes: the second judge of the storage GENERATOR next to the C++ oracle.

    generate(blocks, child_cid, actor_id, slot32) -> (status, claim fields or None, recorded CIDs)

`blocks` is {cid bytes: block bytes}, the RPC blockstore of the reference.  The claim fields are those create_proof_claim
(:158-178) needs: the three derived CIDs (bytes) and the left-padded value — for a failing spec, the CIDs derived before
the Err.  The recorded CIDs are what the reference's three `RecordingBlockStore`s would hold — `get` records a CID whose block exists (common/blockstore.rs:26-30) — in `Cid: Ord`
order (collect_witness_blocks iterates a BTreeSet<Cid>), for failing specs too: everything fetched up to the Err.

The generator's JSON cross-check of parent_state_root (:88-100) has no counterpart: the caller's ApiTipset is not an input.
What this file does not restate (the typed decodes, the HAMT get, the six-way sniff) is pystorage's; see its header for how
far those are independent of the oracle and the engine."""
import pystorage as ps

TRUE = ps.TRUE


class Recorder:
    """`RecordingBlockStore` over a dict: the two things pystorage asks of a store — `cid in blocks`, `blocks[cid]`."""

    def __init__(self, blocks):
        self.blocks = blocks
        self.seen = set()

    def __contains__(self, cid):
        return cid in self.blocks

    def __getitem__(self, cid):
        self.seen.add(cid)
        return self.blocks[cid]

    def get(self, cid):
        """→ the block's bytes or None; a block that exists is recorded"""
        return self[cid] if cid in self.blocks else None


def cid_ord(cid: bytes):
    """The key `#[derive(Ord)]` of cid::Cid compares: version, codec, multihash (code, size, digest)."""
    if len(cid) == 34 and cid[0] == 0x12 and cid[1] == 0x20:
        return (0, 0x70, 0x12, 32, cid[2:])
    ver, pos = ps._varint(cid, 0)
    codec, pos = ps._varint(cid, pos)
    code, pos = ps._varint(cid, pos)
    size, pos = ps._varint(cid, pos)
    return (ver, codec, code, size, cid[pos:])


def cid_of_slot(slot40) -> bytes:
    """The CID a zero-padded 40-byte slot holds (a CID is self-delimiting; its last byte may be zero)."""
    b = bytes(slot40)
    if b[0] == 0x12 and b[1] == 0x20:
        return b[:34]
    pos = 0
    for _ in range(3):
        _v, pos = ps._varint(b, pos)
    size, pos = ps._varint(b, pos)
    return b[: pos + size]


def _generate(rec, child, actor_id, slot32, out):
    # Step 1: extract_and_verify_parent_state (:72-103)
    hdr = rec.get(child)
    if hdr is None:
        raise ps.Err(ps.ERR_MISSING_BLOCK, "missing child header")                  # :81-83
    sroot = out["parent_state_root"] = ps.header_parent_state_root(hdr)             # :86
    # Step 3: load_actor_and_storage_root (:106-134) → get_actor_state (common/decode.rs:17-42)
    raw = rec.get(sroot)
    if raw is None:
        raise ps.Err(ps.ERR_MISSING_BLOCK, "StateRoot")                             # decode.rs:23-25
    actors = ps.state_root_actors(raw)
    n, key = actor_id, bytearray(b"\0")
    while True:                                                                     # Address::new_id(n).to_bytes()
        key.append((n & 0x7F) | (0x80 if n >> 7 else 0))
        n >>= 7
        if not n:
            break
    actor = ps.hamt_get(rec, actors, 5, bytes(key), ps.check_actor_state)
    if actor is None:
        raise ps.Err(ps.ERR_ACTOR_NOT_FOUND, "actor not found")                     # decode.rs:39
    astate = out["actor_state_cid"] = actor[1].cid                                  # :118
    evm = rec.get(astate)
    if evm is None:
        raise ps.Err(ps.ERR_MISSING_BLOCK, "missing EVM state")                     # :121-123
    root = out["storage_root"] = ps.evm_contract_state(evm)                         # :125-126
    # Step 4: read_storage_value (:137-155)
    value = ps.read_storage_slot(rec, root, slot32) or b""                          # :147-148
    out["value"] = ps.left_pad_32(value)


def generate(blocks, child_cid: bytes, actor_id: int, slot32: bytes):
    rec = Recorder(blocks)
    out, st = {}, TRUE  # (a failing spec keeps what was derived before the Err: "storage_root" present ⇔ the chain held)
    try:
        _generate(rec, child_cid, actor_id, slot32, out)
    except ps.Err as e:
        st = e.status
    return st, out, sorted(rec.seen, key=cid_ord)


def spec_of(claim):
    """The (child CID, actor id, slot) a verifier's claim dict poses to the generator, or None where it poses none: the child
    CID must parse and the slot must be 64 hex digits."""
    try:
        child = ps.cid_from_string(claim["child_block_cid"])
    except ValueError:
        return None
    s = claim["slot"]
    while s.startswith("0x"):
        s = s[2:]
    if len(s) != 64 or any(ch not in "0123456789abcdefABCDEF" for ch in s):
        return None
    return child, int(claim["actor_id"]), bytes.fromhex(s)
