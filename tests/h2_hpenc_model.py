"""A sequential model of the header-block encoder (grdma_h2_hpenc, csrc/grdma_h2_hpenc.h): the rules of
include/grdma_amd.h ("Header blocks, sending") applied to a block table, a field table and a string arena -- the layout
the header decoder writes -- giving the exact wire bytes of the HEADERS and CONTINUATION frames, the block-wire table, the
result block, the table and the counters.  tests/test_h2_hpenc_model.py holds it against RFC 7541 Appendix C.4 and C.6,
against the decoder's model (tests/h2_hpack_model.py) and against nghttp2 before a device test trusts it."""
import copy

from tests.h2_hpack_data import HUFFMAN, STATIC
from tests.h2_hpack_model import RingLayout

BAD_INPUT = 1                                                      # GRDMA_H2_HPENC_BAD_INPUT
ERR_FIELD_RANGE, ERR_STREAM, ERR_LENGTH, ERR_STRING, ERR_BLOCK_TOO_LARGE = range(1, 6)  # GRDMA_H2_HPENC_ERR_*
MAX_TABLE, RING, BYTES, CHUNK = 65536, 2048, 65536, 256            # H2HP_MAX_TABLE, H2HP_RING, H2HP_BYTES, H2HE_CHUNK
STAT_KEYS = ("calls", "blocks", "fields", "list_bytes", "wire_bytes", "inserted", "evicted")


def hash_bytes(data, h=0x811c9dc5):
    """FNV-1a, 32 bits: the hash of the device's candidate search.  The name hash is hash_bytes(name), the full hash
    hash_bytes(value, hash_bytes(name)); equal hashes only ever nominate a candidate, the bytes decide."""
    for b in data:
        h = ((h ^ b) * 0x01000193) & 0xffffffff
    return h


def name_hash(name):
    return hash_bytes(name)


def full_hash(name, value):
    return hash_bytes(value, hash_bytes(name))


def enc_int(value, nbits, first=0):
    limit = (1 << nbits) - 1
    if value < limit:
        return bytes([first | value])
    out, rest = [first | limit], value - limit
    while rest >= 128:
        out.append(0x80 | (rest & 0x7f))
        rest >>= 7
    out.append(rest)
    return bytes(out)


def huffman_len(data):
    return (sum(HUFFMAN[b][1] for b in data) + 7) // 8


def enc_str(data):
    """Huffman-coded where that is not longer than the raw bytes (RFC 7541 C.6.2 codes "307" in three bytes), padded
    with one-bits; the empty string goes raw"""
    n = huffman_len(data)
    if n > len(data) or not data:
        return enc_int(len(data), 7, 0) + bytes(data)
    acc = bits = 0
    for b in data:
        code, ln = HUFFMAN[b]
        acc, bits = (acc << ln) | code, bits + ln
    fill = (-bits) % 8
    acc = (acc << fill) | ((1 << fill) - 1)
    return enc_int(n, 7, 0x80) + acc.to_bytes(n, "big")


_STATIC_FULL, _STATIC_NAME = {}, {}
for _i in range(61, 0, -1):  # (the lowest index stays)
    _STATIC_FULL[STATIC[_i]] = _i
    _STATIC_NAME[STATIC[_i][0]] = _i


class EncTable:
    """the encoder's view of the peer's dynamic table: entries newest first"""

    def __init__(self, max_size):
        self.max_size, self.entries, self.size, self.inserted, self.evicted = max_size, [], 0, 0, 0

    def evict(self, need):
        while self.entries and self.size + need > self.max_size:
            n, v = self.entries.pop()
            self.size -= 32 + len(n) + len(v)
            self.evicted += 1

    def resize(self, n):
        self.max_size = n
        self.evict(0)

    def full(self, name, value):
        i = _STATIC_FULL.get((name, value))
        if i:
            return i
        try:
            return 62 + self.entries.index((name, value))  # (the newest)
        except ValueError:
            return 0

    def name(self, name):
        i = _STATIC_NAME.get(name)
        if i:
            return i
        for k, e in enumerate(self.entries):
            if e[0] == name:
                return 62 + k
        return 0

    def field(self, name, value, hint):
        """-> (the field's bytes, its representation: 0 indexed, 1 incremental, 2 without indexing, 3 never indexed)"""
        hint &= 3
        if hint != 3:
            i = self.full(name, value)
            if i:
                return enc_int(i, 7, 0x80), 0
        i = self.name(name)  # (in front of the evictions: RFC 7541 4.4)
        rep = 1 if hint < 2 else hint
        first, nbits = {1: (0x40, 6), 2: (0x00, 4), 3: (0x10, 4)}[rep]
        out = enc_int(i, nbits, first) + (b"" if i else enc_str(name)) + enc_str(value)
        if rep == 1:
            need = 32 + len(name) + len(value)
            self.evict(need)
            if need <= self.max_size:
                self.entries.insert(0, (name, value))
                self.size += need
                self.inserted += 1
        return out, rep


def frames(stream, end_stream, payload, max_frame):
    """one HEADERS frame, then CONTINUATION frames of max_frame bytes; END_HEADERS on the last -> (bytes, frames)"""
    parts = [payload[i:i + max_frame] for i in range(0, len(payload), max_frame)] or [b""]
    out = bytearray()
    for k, p in enumerate(parts):
        fl = (4 if k == len(parts) - 1 else 0) | (1 if k == 0 and end_stream else 0)
        out += len(p).to_bytes(3, "big") + bytes([1 if k == 0 else 9, fl]) + stream.to_bytes(4, "big") + p
    return bytes(out), len(parts)


class HpencModel:
    def __init__(self, peer_table=4096, peer_max_frame=16384):
        # (what both sides hold before any SETTINGS: 4096; a peer that announced more is told so in the first block)
        self.table = EncTable(min(peer_table, 4096))
        self.want = self.low = peer_table if peer_table > 4096 else self.table.max_size
        self.low = min(self.low, self.table.max_size)
        self.max_frame = peer_max_frame
        self.stats = dict.fromkeys(STAT_KEYS, 0)
        self.last_reps = []

    def set_peer(self, peer_table, peer_max_frame):
        self.want, self.low, self.max_frame = peer_table, min(self.low, peer_table), peer_max_frame

    def updates(self):
        cur = self.table.max_size
        if self.low < self.want and self.low < cur:
            return [self.low, self.want]
        return [self.want] if self.want != cur else []

    def _check(self, k, blocks, fields, arena_len):
        stream, first, n, _ = blocks[k]
        if first + n > len(fields):
            return ERR_FIELD_RANGE
        if stream == 0 or stream > 0x7fffffff:
            return ERR_STREAM
        for no, vo, nl, vl in fields[first:first + n]:
            if vl > 0xffffff:
                return ERR_LENGTH
            if no + (nl & 0xffffff) > arena_len or vo + vl > arena_len:
                return ERR_STRING
        return 0

    def encode(self, blocks, fields, arena, wire_cap, bw_cap):
        """blocks [(stream, first field, fields, flags)], fields [(name offset, value offset, name length | hint << 24,
        value length)], the string arena -> (wire bytes, block-wire table [(offset, length, frames)], result tuple,
        the error the call raises: None | "capacity" | "invalid")"""
        self.last_reps = reps = []
        for k in range(len(blocks)):
            err = self._check(k, blocks, fields, len(arena))
            if err:
                return b"", [], (0, 0, 0, 0, 0, self.table.size, BAD_INPUT | err << 8 | k << 32, 0), "invalid"
        t = copy.deepcopy(self.table)
        ins0, ev0 = t.inserted, t.evicted
        wire, bw, nframes, list_bytes, nfields = bytearray(), [], 0, 0, 0
        for k, (stream, first, n, flags) in enumerate(blocks):
            payload = bytearray()
            if k == 0:
                for u in self.updates():
                    payload += enc_int(u, 5, 0x20)
                    t.resize(u)
            for no, vo, nl, vl in fields[first:first + n]:
                name, value = bytes(arena[no:no + (nl & 0xffffff)]), bytes(arena[vo:vo + vl])
                b, rep = t.field(name, value, nl >> 24)
                payload += b
                reps.append(rep)
                list_bytes += len(name) + len(value)
            nfields += n
            fr, nf = frames(stream, flags & 1, bytes(payload), self.max_frame)
            if len(fr) > 0xffffffff:
                return b"", [], (0, 0, 0, 0, 0, self.table.size, BAD_INPUT | ERR_BLOCK_TOO_LARGE << 8 | k << 32, 0), "invalid"
            bw.append((len(wire), len(fr), nf))
            wire += fr
            nframes += nf
        res = (len(blocks), nframes, len(wire), t.inserted - ins0, t.evicted - ev0, t.size, 0)
        if len(wire) > wire_cap or len(blocks) > bw_cap:
            return b"", [], res + (1,), "capacity"
        self.table = t
        if blocks:
            self.want = self.low = t.max_size
        st = self.stats
        st["calls"] += 1
        st["blocks"] += len(blocks)
        st["fields"] += nfields
        st["list_bytes"] += list_bytes
        st["wire_bytes"] += len(wire)
        st["inserted"] += res[3]
        st["evicted"] += res[4]
        return bytes(wire), bw, res + (0,), None


# ---- what the encoder's stages see of a call, from the model alone (the witnesses of tests/h2_hpenc_sweep_lib.py) ------
# Nothing here decides a byte: the facts are read off the model's own sequential run (EncTable.field, one occurrence
# after the other) and off the bytes it gave.
def first_int(data, nbits):
    """the prefix integer a field's bytes begin with"""
    limit = (1 << nbits) - 1
    v = data[0] & limit
    if v < limit:
        return v
    k = 1
    while True:
        v += (data[k] & 0x7f) << (7 * (k - 1))
        if not data[k] & 0x80:
            return v
        k += 1


def occurrences(blocks):
    """a good call's occurrences in wire order -> [(block, field index)]"""
    return [(k, first + j) for k, (_, first, n, _) in enumerate(blocks) for j in range(n)]


def trace(model, blocks, fields, arena):
    """a call the model takes (no bad input), replayed on a copy of its table -> dict(occ: per occurrence (its step of
    the walk, its representation, the index its bytes begin with, whether it is taken by the one inserting thread --
    an entry larger than the table is, and inserts nothing --, the entries it evicted, whether it inserted), steps: per
    step the inserting occurrences in order [(occurrence, evicted, inserted)], updates: the size updates in front)"""
    t, occ, steps = copy.deepcopy(model.table), [], {}
    ups = model.updates() if blocks else []
    for u in ups:
        t.resize(u)
    for i, (_, fi) in enumerate(occurrences(blocks)):
        no, vo, nl, vl = fields[fi]
        ins0, ev0 = t.inserted, t.evicted
        b, rep = t.field(bytes(arena[no:no + (nl & 0xffffff)]), bytes(arena[vo:vo + vl]), nl >> 24)
        o = (i // CHUNK, rep, first_int(b, (7, 6, 4, 4)[rep]), rep == 1, t.evicted - ev0, t.inserted > ins0)
        occ.append(o)
        if o[3]:
            steps.setdefault(o[0], []).append((i, o[4], o[5]))
    return dict(occ=occ, steps=steps, updates=ups)


def live(table):
    """-> every live entry's (insertion number since creation, ring slot), newest first"""
    return [(table.inserted - 1 - k, (table.inserted - 1 - k) % RING) for k in range(len(table.entries))]


class ByteRing(RingLayout):
    """the decoder's RingLayout over an EncTable (the head advances by the string bytes of the entries a call inserted
    and that survive it, in insertion order, modulo BYTES; straddles(): which live strings lie across BYTES, and in
    which part), and the bytes the ring then holds"""

    def __init__(self):
        RingLayout.__init__(self)
        self.bytes = bytearray(BYTES)

    def commit(self, table, inserted):
        RingLayout.commit(self, table, inserted)
        for (off, nl, vl), (name, value) in list(zip(self.where, table.entries))[:min(inserted, len(table.entries))]:
            for k, b in enumerate(name + value):
                self.bytes[(off + k) % BYTES] = b


def pack(lists, hints=None):
    """header lists [(stream, flags, [(name, value[, hint])])] -> (blocks, fields, arena) in the decoder's layout"""
    blocks, fields, arena = [], [], bytearray()
    for stream, flags, hs in lists:
        first = len(fields)
        for h in hs:
            name, value = h[0], h[1]
            hint = h[2] if len(h) > 2 else 1
            fields.append((len(arena), len(arena) + len(name), len(name) | hint << 24, len(value)))
            arena += name + value
        blocks.append((stream, first, len(hs), flags))
    return blocks, fields, bytes(arena)


def deframe(wire):
    """the frames of an encoder's output -> [(stream, end_stream, block)]"""
    out, pos, cur = [], 0, None
    while pos < len(wire):
        n, t, fl, sid = int.from_bytes(wire[pos:pos + 3], "big"), wire[pos + 3], wire[pos + 4], int.from_bytes(wire[pos + 5:pos + 9], "big")
        body = wire[pos + 9:pos + 9 + n]
        if t == 1:
            if cur is not None:
                raise ValueError("HEADERS inside an open block")
            cur = [sid, fl & 1, bytearray(body)]
        elif t == 9 and cur is not None and sid == cur[0]:
            cur[2] += body
        else:
            raise ValueError("frame type %d at %d" % (t, pos))
        if fl & 4:
            out.append((cur[0], cur[1], bytes(cur[2])))
            cur = None
        pos += 9 + n
    if cur is not None or pos != len(wire):
        raise ValueError("the wire ends inside a block")
    return out
