"""What the pair-level device tests share: a connected loop-back link, the protocol state compared with the oracle's,
ring and staging images compared up to their pad bytes (tests/test_gpu_pair_parity.py and the files that build on
it), and the replay of a golden trace on anything with the oracle link's methods (tests/test_golden_ring.py on the
oracle, tests/test_gpu_pair_parity.py on the HIP pair)."""
import hashlib
import random

STATE_KEYS = ["head", "moving_head", "remain", "remote_tail", "remote_head",
              "internal_read_size", "credit_msgs", "partial_write"]


def mk_link(g, R, sge, flags=0):
    a, b = g.Pair(R, sge, flags), g.Pair(R, sge, flags)
    g.connect_pairs(a, b)
    return a, b


def check_state(a, b, o):
    sa, sb = a.state(), b.state()
    oa, ob = o.state(0), o.state(1)
    for k in STATE_KEYS:
        assert sa[k] == oa[k], ("side0", k, sa, oa)
        assert sb[k] == ob[k], ("side1", k, sb, ob)


def _records(buf):
    """Yield (offset, payload_len) of back-to-back records in a staging image."""
    off = 0
    while off + 16 <= len(buf):
        n = int.from_bytes(buf[off:off + 8], "little")
        if n == 0:
            break
        yield off, n
        off += 16 + ((n + 7) & ~7)


def _mask_pads(buf):
    out = bytearray(buf)
    for off, n in _records(buf):
        for q in range(off + 8 + n, off + 8 + ((n + 7) & ~7)):
            out[q] = 0
    return bytes(out)


def _ring_eq(x, y):
    # Oracle staging starts zeroed and both sides see the same send history, but
    # the oracle's pad bytes can hold stale bytes of an earlier, longer record.
    # Compare everything except pad bytes, which are located from the record tags
    # still in the ring (both images must agree on every tag word).
    if x == y:
        return True
    R = len(x)
    diff = [i for i in range(R) if x[i] != y[i]]
    # every differing byte must be a pad byte: the HIP side holds 0 there
    for i in diff:
        if x[i] != 0:
            return False
        w = i & ~7
        # pad bytes live in the last payload word of a record: the next word is the footer
        nxt = (w + 8) % R
        if x[nxt:nxt + 8] != b"\xff" * 8 or y[nxt:nxt + 8] != b"\xff" * 8:
            return False
    return True


def payload(seed, n):
    rng = random.Random(seed)
    return bytes(rng.getrandbits(8) for _ in range(n))


def sha(b):
    return hashlib.sha256(b).hexdigest()


def replay(doc, link, ring_exact=True, mask=None):
    for i, st in enumerate(doc["steps"]):
        if st["op"] == "send":
            sl = [payload(s, n) for s, n in st["slices"]]
            assert link.send(0, sl, st.get("byte_idx", 0)) == st["sent"], (doc["name"], i)
            assert [list(w) for w in link.last_wrs(0)] == st["wrs"]
            if ring_exact:
                assert sha(link.staging_mem(0)) == st["staging_sha256"]
        elif st["op"] == "recv":
            got = link.recv(1, st["cap"])
            assert len(got) == st["got_len"] and sha(got) == st["got_sha256"]
        else:
            got, alloc = link.endpoint_read(1)
            assert len(got) == st["got_len"] and sha(got) == st["got_sha256"]
            assert alloc == st["alloc"]
        if ring_exact:
            assert sha(link.ring_mem(1)) == st["ring_sha256"], (doc["name"], i)
        elif "ring_hex" in st:
            assert mask(link.ring_mem(1), bytes.fromhex(st["ring_hex"])), (doc["name"], i)
        rx, tx = link.state(1), link.state(0)
        for k, v in st["rx_state"].items():
            assert rx[k] == v, (doc["name"], i, "rx", k)
        for k, v in st["tx_state"].items():
            assert tx[k] == v, (doc["name"], i, "tx", k)
        assert link.readable(1) == st["readable"]
        assert link.has_message(1) == st["has_message"]
        assert link.writable(0) == st["writable"]
