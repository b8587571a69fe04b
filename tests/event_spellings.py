"""StampedEvent encoders and the list of StampedEvent SPELLINGS (repeated keys, entries the fast decode declines, every
emitter width, data of 0 … 70000 bytes) that tests/test_gpu_generate_claims.py lowers on raw blocks and
tests/event_chain_cases.py wraps into events AMTs for the verifier, the table parse and the scan."""
import numpy as np

from pyamt import array, bstr, head, uint


def text(s: str) -> bytes:
    b = s.encode()
    return head(3, len(b)) + b


def entry(key: str, value: bytes, flags: int = 3, codec: int = 0x55) -> bytes:
    return array([uint(flags), text(key), uint(codec), bstr(value)])


def stamped(emitter: int, entries) -> bytes:
    return array([uint(emitter), array(list(entries))])


def topic(k: int) -> bytes:
    return bytes((k * 37 + i) & 0xFF for i in range(32))


def data_bytes(n: int, salt: int = 0) -> bytes:
    return (np.arange(n, dtype=np.uint32) * 7 + salt).astype(np.uint8).tobytes()


def spelling_cases():
    """[(name, StampedEvent bytes, emitter, expected to be a bad record)]"""
    T = [topic(k) for k in range(1, 10)]
    cases = []

    def add(name, entries, emitter=None, bad=False):
        emitter = 1000 + len(cases) if emitter is None else emitter
        cases.append((name, stamped(emitter, entries), emitter, bad))

    # Case B
    for n in (1, 2, 3, 4):
        add(f"B {n} topics", [entry(f"t{k + 1}", T[k]) for k in range(n)] + [entry("d", data_bytes(40, n))])
    add("B t1 t2 t4: stops at 2", [entry("t1", T[0]), entry("t2", T[1]), entry("t4", T[3]), entry("d", b"\x01\x02")])
    add("B t5 is ignored", [entry(f"t{k + 1}", T[k]) for k in range(5)] + [entry("d", b"\x05")])
    add("B no d", [entry("t1", T[0]), entry("t2", T[1])])
    for n in (0, 1, 23, 24, 31, 32, 33, 255, 256, 257, 65535, 65536, 70000):
        add(f"B d of {n}", [entry("t1", T[0]), entry("t2", T[2]), entry("d", data_bytes(n, n))])
    # Case A: the count comes from the value's length
    for n in (0, 32, 64, 128, 160, 288):
        cat = b"".join(T[k] for k in range(n // 32))
        add(f"A topics of {n} with data", [entry("topics", cat), entry("data", data_bytes(50 + n, 3))])
        add(f"A topics of {n} without data", [entry("topics", cat)])
    add("A wins over t1", [entry("t1", T[5]), entry("topics", T[0] + T[1]), entry("d", b"\xdd" * 9), entry("data", b"\xaa" * 5)])
    # repeated keys: the last one wins
    add("repeated t1 and d", [entry("t1", T[0]), entry("d", b"first"), entry("t1", T[4]), entry("t2", T[1]), entry("d", b"the last")])
    add("repeated topics", [entry("topics", T[0]), entry("data", b"x"), entry("topics", T[1] + T[2] + T[3]), entry("data", b"yy")])
    add("repeated t1: the last one spoils it", [entry("t1", T[0]), entry("t1", T[1][:31])], bad=True)
    # the emitter in every width
    for em in (0, 23, 24, 255, 256, 65536, 1 << 32, (1 << 64) - 1):
        add(f"emitter {em}", [entry("t1", T[0]), entry("t2", T[1]), entry("d", b"\x07" * 3)], emitter=em)
    # entries the fast entry decode declines (a 7-byte key, flags >= 24) among the ones that matter
    add("declined entries", [entry("ignored", b"zz"), entry("t1", T[0], flags=24), entry("longkey", T[1]), entry("t2", T[1], flags=200),
                             entry("d", data_bytes(70, 9), flags=0x1234, codec=0x12345)])
    # extract_evm_log is None
    add("t1 of 31 bytes", [entry("t1", T[0][:31]), entry("d", b"\x01")], bad=True)
    add("topics of 40 bytes", [entry("topics", T[0] + T[1][:8]), entry("data", b"\x01")], bad=True)
    add("no topic key", [entry("d", b"\x01\x02\x03"), entry("data", b"\x04")], bad=True)
    add("t2 of 33 bytes behind a good t1", [entry("t1", T[0]), entry("t2", T[1] + b"\0")], bad=True)
    return cases
