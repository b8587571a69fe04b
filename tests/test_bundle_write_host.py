"""CPU: the host half of the bundle WRITER (csrc/host/bundle_write.cpp, ipcfp_bundle_write_claims_json — no GPU involved):
claim structs → `{"storage_proofs":[…],"event_proofs":[…],"blocks":[`, byte for byte what serde_json::to_string writes.
The expected text comes from tests/bundle_ref.py's writer, and from json.dumps(ensure_ascii=False, separators=(",", ":"))
— serde_json's escaping rule — where escapes matter; never from the code under test."""
import ctypes as C
import os

import pytest

import bundle_ref
import ipc_filecoin_proofs_amd as ipcfp
from bundle_write_cases import arrays, event_proof, head_text, storage_proof

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bundle_small.json")
E_INVALID = -1

def write(storage, events) -> bytes:
    st, ev = arrays(storage, events)
    return ipcfp.bundle_claims_json(st.arr, st.n, ev.arr, ev.n)


def raw_call(st, ev, out, cap):
    lib = ipcfp.load_library()
    n = C.c_uint64(0xDEAD)
    rc = lib.ipcfp_bundle_write_claims_json(C.cast(st.arr, C.c_void_p), st.n, C.cast(ev.arr, C.c_void_p), ev.n, out, cap, C.byref(n))
    return rc, int(n.value)


def test_golden_fixture_head():
    text = open(GOLDEN, "rb").read()
    parsed = bundle_ref.parse_bundle(text)
    assert len(parsed["event_proofs"]) == 7 and len(parsed["storage_proofs"]) == 9
    cut = text.index(b'"blocks":[') + len(b'"blocks":[')
    assert write(parsed["storage_proofs"], parsed["event_proofs"]) == text[:cut]
    # the restated writer agrees with the fixture, so it can stand as the reference elsewhere
    assert bundle_ref.bundle_json(parsed["storage_proofs"], parsed["event_proofs"], parsed["blocks"]).encode() == text


def test_escapes_follow_serde_json():
    every = "".join(chr(c) for c in range(1, 0x80))
    tricky = 'q"b\\s/\u00e9\u2028\U0001F600'
    storage = [storage_proof(child_block_cid=every, parent_state_root=tricky, value=every[::-1] + tricky)]
    events = [event_proof(parent_tipset_cids=[every[:0x40], every[0x40:], tricky], message_cid=tricky + every,
                          topics=[tricky, every], data=every + tricky)]
    got = write(storage, events)
    assert got == head_text(storage, events)
    for needle in (b"\\u0001", b"\\u001f", b"\\b", b"\\t", b"\\n", b"\\f", b"\\r", b'\\"', b"\\\\", b"/", b"\x7f",
                   "\u00e9\u2028\U0001F600".encode()):
        assert needle in got
    assert b"\\/" not in got and b"\\u007f" not in got and b"\\u2028" not in got
    # json.dumps' default is NOT this rule (it escapes 0x7f upward): the two references differ on this input
    assert got != bundle_ref.bundle_json(storage, events, []).encode()[: len(got)]


def test_integer_extremes():
    storage = [storage_proof(child_epoch=-(1 << 63), actor_id=(1 << 64) - 1), storage_proof(child_epoch=(1 << 63) - 1, actor_id=0),
               storage_proof(child_epoch=-1)]
    events = [event_proof(parent_epoch=-(1 << 63), child_epoch=(1 << 63) - 1, exec_index=(1 << 64) - 1, event_index=0,
                          emitter=(1 << 64) - 1), event_proof(parent_epoch=-1, child_epoch=0, exec_index=0, emitter=0)]
    got = write(storage, events)
    assert got == head_text(storage, events)
    assert b"-9223372036854775808" in got and b"18446744073709551615" in got and b'"child_epoch":-1,' in got


def test_zero_parents_and_zero_topics():
    events = [event_proof(parent_tipset_cids=[], topics=[]), event_proof(parent_tipset_cids=[]), event_proof(topics=[])]
    got = write([], events)
    assert got == head_text([], events)
    assert b'"parent_tipset_cids":[],' in got and b'"topics":[],' in got


def test_both_lists_empty():
    assert write([], []) == b'{"storage_proofs":[],"event_proofs":[],"blocks":['
    lib = ipcfp.load_library()
    n = C.c_uint64()
    assert lib.ipcfp_bundle_write_claims_json(None, 0, None, 0, None, 0, C.byref(n)) == 0 and n.value == 49


@pytest.mark.parametrize("bad", [b"\xff", b"ab\x80cd", b"abc\xe2\x82", b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"],
                         ids=["ff", "lone-continuation", "truncated", "overlong", "surrogate", "above-10ffff"])
def test_invalid_utf8_is_refused(bad):
    for which in ("storage.slot", "event.message_cid", "event.topic", "event.parent"):
        st, ev = arrays([storage_proof(), storage_proof()], [event_proof(), event_proof()])
        if which == "storage.slot":
            st.arr[1].slot = bad
        elif which == "event.message_cid":
            ev.arr[1].message_cid = bad
        elif which == "event.topic":
            ev.arr[0].topics[1] = bad
        else:
            ev.arr[1].parent_tipset_cids[0] = bad
        assert raw_call(st, ev, None, 0)[0] == E_INVALID, which
        buf = C.create_string_buffer(b"\xa5" * 4096, 4096)
        assert raw_call(st, ev, C.cast(buf, C.c_void_p), 4096)[0] == E_INVALID, which
        assert buf.raw == b"\xa5" * 4096
    st, ev = arrays([storage_proof()], [event_proof()])
    assert raw_call(st, ev, None, 0)[0] == 0


def test_null_field_pointers_are_refused():
    for field in ("child_block_cid", "parent_state_root", "actor_state_cid", "storage_root", "slot", "value"):
        st, ev = arrays([storage_proof(), storage_proof()], [])
        setattr(st.arr[1], field, None)
        assert raw_call(st, ev, None, 0)[0] == E_INVALID, field
    for field in ("child_block_cid", "message_cid", "data"):
        st, ev = arrays([], [event_proof()])
        setattr(ev.arr[0], field, None)
        assert raw_call(st, ev, None, 0)[0] == E_INVALID, field
    st, ev = arrays([], [event_proof()])
    ev.arr[0].topics[0] = None
    assert raw_call(st, ev, None, 0)[0] == E_INVALID
    st, ev = arrays([], [event_proof()])
    ev.arr[0].parent_tipset_cids = C.POINTER(C.c_char_p)()  # n_parent_tipset_cids stays 2
    assert raw_call(st, ev, None, 0)[0] == E_INVALID
    # a null array with a count, and a null output with a capacity
    lib = ipcfp.load_library()
    n = C.c_uint64()
    assert lib.ipcfp_bundle_write_claims_json(None, 1, None, 0, None, 0, C.byref(n)) == E_INVALID
    assert lib.ipcfp_bundle_write_claims_json(None, 0, None, 0, None, 10, C.byref(n)) == E_INVALID


def test_buffer_contract():
    storage, events = [storage_proof(), storage_proof(value="0x" + "22" * 32)], [event_proof(), event_proof(topics=[])]
    want = head_text(storage, events)
    st, ev = arrays(storage, events)
    rc, n = raw_call(st, ev, None, 0)
    assert rc == 0 and n == len(want)
    # cap == len: every byte of the text, and the 64 bytes behind it untouched
    buf = C.create_string_buffer(b"\xa5" * (n + 64), n + 64)
    rc, n2 = raw_call(st, ev, C.cast(buf, C.c_void_p), n)
    assert rc == 0 and n2 == n
    assert buf.raw[:n] == want and buf.raw[n:] == b"\xa5" * 64
    # cap == len - 1: refused, *len still set, the whole buffer untouched
    buf = C.create_string_buffer(b"\xa5" * (n + 64), n + 64)
    rc, n3 = raw_call(st, ev, C.cast(buf, C.c_void_p), n - 1)
    assert rc == E_INVALID and n3 == n
    assert buf.raw == b"\xa5" * (n + 64)


def test_one_thread_and_eight_write_the_same_bytes(monkeypatch):
    """20 000 claims: the ranges are sized and written by one thread and by eight (IPCFP_HOST_THREADS pins the count)."""
    storage = [storage_proof(actor_id=1000 + i, child_epoch=i - 4000, slot="0x%064x" % i) for i in range(8000)]
    events = [event_proof(exec_index=i, event_index=i % 7, parent_epoch=-i, topics=["0x%064x" % i] * (i % 4),
                          data="0x" + "ab" * (i % 50), message_cid="bafy-msg-%d\t" % i) for i in range(12000)]
    st, ev = arrays(storage, events)
    monkeypatch.setenv("IPCFP_HOST_THREADS", "1")
    one = ipcfp.bundle_claims_json(st.arr, st.n, ev.arr, ev.n)
    monkeypatch.setenv("IPCFP_HOST_THREADS", "8")
    eight = ipcfp.bundle_claims_json(st.arr, st.n, ev.arr, ev.n)
    monkeypatch.delenv("IPCFP_HOST_THREADS")
    default = ipcfp.bundle_claims_json(st.arr, st.n, ev.arr, ev.n)
    want = head_text(storage, events)
    assert one == want and eight == want and default == want
    # an error in a late range is still found when the ranges are sized in parallel
    monkeypatch.setenv("IPCFP_HOST_THREADS", "8")
    ev.arr[11999].data = b"\xff"
    assert raw_call(st, ev, None, 0)[0] == E_INVALID
