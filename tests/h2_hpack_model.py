"""A sequential model of the header-block decoder (grdma_h2_hpack, csrc/grdma_h2_hpack.h): rules 1 to 6 of
include/grdma_amd.h ("Header blocks") applied to the ORACLE's event list (oracle/pyorc.H2Parser.feed) plus the bytes that
were fed.  The static table and the Huffman code are data (tests/h2_hpack_data.py); tests/test_h2_hpack_model.py pins
them, and the decoding, against nghttp2 and against tests/golden/h2_hpack_vectors.json before a device test trusts them.

A block is decoded in two steps, and a block with more than one fault reports the first fault of the first step:
  split   the field boundaries in wire order: integers, string lengths, Huffman strings, where size updates stand and
          their bound (ERR_INTEGER, ERR_TRUNCATED, ERR_HUFFMAN, ERR_SIZE_UPDATE);
  table   the fields against the dynamic table, in order (ERR_INDEX)."""
import copy

from oracle.pyorc import EV_FRAME, EV_PAYLOAD
from tests.h2_hpack_data import HUFFMAN, STATIC  # [(code, bits)] * 257 (256: EOS); [(name, value)] * 62 (0: unused)

FAILED, LOST, OPEN = 1, 2, 4  # GRDMA_H2_HPACK_*
ERR_PADDING, ERR_BLOCK_TOO_LARGE, ERR_INTEGER, ERR_TRUNCATED, ERR_HUFFMAN, ERR_INDEX, ERR_SIZE_UPDATE, ERR_DEFRAMER = range(1, 9)
HEADERS, CONTINUATION = 1, 9
END_STREAM, END_HEADERS, PADDED, PRIORITY = 1, 4, 8, 0x20
STAT_KEYS = ("calls", "blocks", "fields", "string_bytes", "inserted", "evicted", "flags")
_DECODE = {(ln, code): s for s, (code, ln) in enumerate(HUFFMAN)}


class HpackError(Exception):
    def __init__(self, code):
        Exception.__init__(self, "HPACK error %d" % code)
        self.code = code


def read_int(data, pos, nbits):
    """-> (value, position behind it); at most five continuation bytes, at most 2^32 - 1"""
    if pos >= len(data):
        raise HpackError(ERR_TRUNCATED)
    limit = (1 << nbits) - 1
    v, pos = data[pos] & limit, pos + 1
    if v < limit:
        return v, pos
    for k in range(5):
        if pos >= len(data):
            raise HpackError(ERR_TRUNCATED)
        b, pos = data[pos], pos + 1
        v += (b & 0x7f) << (7 * k)
        if not b & 0x80:
            if v > 0xffffffff:
                raise HpackError(ERR_INTEGER)
            return v, pos
    raise HpackError(ERR_INTEGER)


def huffman_decode(data):
    out, code, ln = bytearray(), 0, 0
    for byte in data:
        for bit in range(7, -1, -1):
            code, ln = (code << 1) | ((byte >> bit) & 1), ln + 1
            s = _DECODE.get((ln, code))
            if s is not None:
                if s == 256:
                    raise HpackError(ERR_HUFFMAN)  # EOS inside a string
                out.append(s)
                code = ln = 0
            elif ln >= 30:
                raise HpackError(ERR_HUFFMAN)
    if ln > 7 or code != (1 << ln) - 1:  # the padding: at most 7 bits, all ones
        raise HpackError(ERR_HUFFMAN)
    return bytes(out)


def read_str(data, pos):
    if pos >= len(data):
        raise HpackError(ERR_TRUNCATED)
    h = data[pos] & 0x80
    n, pos = read_int(data, pos, 7)
    if pos + n > len(data):
        raise HpackError(ERR_TRUNCATED)
    raw = bytes(data[pos:pos + n])
    return (huffman_decode(raw) if h else raw), pos + n


def split(data, setting):
    """the block's fields in wire order: ("size", n) | (representation, index, name or None, value or None);
    representation 0 indexed, 1 incremental, 2 without indexing, 3 never indexed"""
    out, pos, seen_field = [], 0, False
    while pos < len(data):
        b = data[pos]
        if b & 0x80:
            i, pos = read_int(data, pos, 7)
            out.append((0, i, None, None))
            seen_field = True
            continue
        if b & 0xe0 == 0x20:
            n, pos = read_int(data, pos, 5)
            if seen_field or n > setting:
                raise HpackError(ERR_SIZE_UPDATE)
            out.append(("size", n))
            continue
        rep, nbits = (1, 6) if b & 0x40 else (3, 4) if b & 0x10 else (2, 4)
        i, pos = read_int(data, pos, nbits)
        name = None
        if i == 0:
            name, pos = read_str(data, pos)
        value, pos = read_str(data, pos)
        out.append((rep, i, name, value))
        seen_field = True
    return out


class HpackTable:
    """RFC 7541 dynamic table: entries newest first; `setting` is our SETTINGS_HEADER_TABLE_SIZE, the bound of the
    peer's size updates; max_size what the peer's encoder is at (4096 at the start, or the setting where that is less)"""

    def __init__(self, setting=4096):
        self.setting, self.max_size = setting, min(4096, setting)
        self.entries, self.size, self.inserted, self.evicted = [], 0, 0, 0

    def set_setting(self, n):
        """a lowered setting takes effect at once (the table never holds more than we said we keep)"""
        self.setting = n
        if self.max_size > n:
            self.max_size = n
            self._evict(0)

    def _evict(self, need):
        while self.entries and self.size + need > self.max_size:
            n, v = self.entries.pop()
            self.size -= 32 + len(n) + len(v)
            self.evicted += 1

    def get(self, i):
        if i == 0 or i >= 62 + len(self.entries):
            raise HpackError(ERR_INDEX)
        return STATIC[i] if i < 62 else self.entries[i - 62]

    def apply(self, fields):
        """the split fields against the table -> [(name, value, representation)]"""
        out = []
        for f in fields:
            if f[0] == "size":
                self.max_size = f[1]
                self._evict(0)
                continue
            rep, i, name, value = f
            if rep == 0:
                name, value = self.get(i)
            elif i:
                name = self.get(i)[0]  # (resolved before the insertion evicts: RFC 7541 4.4)
            if rep == 1:
                need = 32 + len(name) + len(value)
                self._evict(need)
                if need <= self.max_size:
                    self.entries.insert(0, (name, value))
                    self.size += need
                    self.inserted += 1
            out.append((name, value, rep))
        return out

    def decode_block(self, data):
        return self.apply(split(data, self.setting))


# ---- what the decoder's stages see of a call, from the model alone (the witnesses of tests/h2_hpack_sweep_lib.py) ------
THREADS, CHUNK, RING, BYTES = 256, 512, 2048, 65536  # H2HP_THREADS, H2HP_CHUNK, H2HP_RING, H2HP_BYTES of csrc/grdma_h2_hpack.h


def block_facts(data, setting):
    """-> (records, fields, size updates) of a block the split takes, None of one it refuses"""
    try:
        fs = split(data, setting)
    except HpackError:
        return None
    su = sum(1 for f in fs if f[0] == "size")
    return len(fs), len(fs) - su, su


def walk_steps(nrecs):
    """the records per block of the blocks a call delivers -> the walk's steps [(first block, blocks taken whole,
    first record, records)]: as many whole blocks (one a thread: THREADS at most) as sum to <= CHUNK records, else
    CHUNK records of one block (blocks taken whole: 0)"""
    out, k = [], 0
    while k < len(nrecs):
        m = tot = 0
        while k + m < len(nrecs) and m < THREADS and tot + nrecs[k + m] <= CHUNK:
            tot, m = tot + nrecs[k + m], m + 1
        if m:
            out.append((k, m, 0, tot))
            k += m
        else:
            out += [(k, 0, f0, min(CHUNK, nrecs[k] - f0)) for f0 in range(0, nrecs[k], CHUNK)]
            k += 1
    return out


def gather_steps(nevents):
    """items per step of the gather: item 0 is the carried frame and block, item t event t - 1"""
    return [min(THREADS, nevents + 1 - c0) for c0 in range(0, nevents + 1, THREADS)]


def header_items(events, carried):
    """the item numbers of a call's header frames (the carried block's is 0)"""
    return ([0] if carried else []) + [t + 1 for t, e in enumerate(events) if e[0] == EV_FRAME and e[1] in (HEADERS, CONTINUATION)]


class RingLayout:
    """Where the device keeps the strings of the dynamic table: per committed call the byte ring's head advances by the
    string bytes of the entries inserted in that call that are alive at its end, oldest first, mod BYTES; descriptor i
    (the i-th insertion since creation) stands in slot i mod RING."""

    def __init__(self):
        self.head = 0
        self.where = []  # newest first, beside HpackTable.entries: (offset, name length, value length)

    def commit(self, table, inserted):
        """behind a committed call that made `inserted` insertions (or a resize: 0)"""
        fresh = min(inserted, len(table.entries))
        new = []
        for name, value in reversed(table.entries[:fresh]):
            new.insert(0, (self.head, len(name), len(value)))
            self.head = (self.head + len(name) + len(value)) % BYTES
        self.where = new + self.where[:len(table.entries) - fresh]

    def straddles(self):
        """which live strings lie across offset BYTES: [(index from 62, "name" | "value" | "between")]; between: the name
        ends and the value begins there"""
        out = []
        for i, (a, nl, vl) in enumerate(self.where):
            b, c = a + nl, a + nl + vl
            if a < BYTES < b:
                out.append((62 + i, "name"))
            if nl and vl and b == BYTES:
                out.append((62 + i, "between"))
            if b < BYTES < c:
                out.append((62 + i, "value"))
        return out


class HpackModel:
    closed = ()  # the blocks the last call completed, delivered or not: their bytes

    def __init__(self, setting=4096, max_block=65536):
        self.table = HpackTable(setting)
        self.max_block = max_block
        self.frame = None   # the open frame: dict(type, flags, size, seen, pad)
        self.block = None   # the open block: dict(stream, flags, frag)
        self.word = 0       # flags | error << 8 | stream << 32, sticky
        self.stats = dict.fromkeys(STAT_KEYS, 0)

    def set_max_table_size(self, n):
        before = self.table.evicted
        self.table.set_setting(n)
        self.stats["evicted"] += self.table.evicted - before

    def _dead(self, word, overflow, rc):
        self.word |= word
        self.frame = self.block = None
        self.stats["calls"] += 1
        self.stats["flags"] = self.word
        self.closed = []
        return [], [], b"", (0, 0, 0, 0, 0, self.table.size, self.word, overflow), rc

    def decode(self, events, slices, err, caps, skipped=False, lost=False):
        """events: the oracle's, tagged with the slice index; slices: the bytes fed; caps: (blocks, fields, string bytes)
        -> (blocks [(stream, first field, fields, flags)], fields [(name offset, value offset, name length |
        representation << 24, value length)], string arena, result tuple, whether the call raises -GRDMA_ERR_CAPACITY)"""
        if self.word & (FAILED | LOST):
            return self._dead(0, 0, False)
        if lost:
            return self._dead(LOST, 2, True)
        if skipped:
            return self._dead(LOST, 0, False)
        if err:
            return self._dead(FAILED | ERR_DEFRAMER << 8, 0, False)
        self.closed = closed = []
        m = copy.deepcopy(self)  # (nothing is committed when a cap overflows)
        blocks, fields, strings, failure = [], [], bytearray(), 0
        ins0, ev0 = m.table.inserted, m.table.evicted
        try:
            for k, a, b, c, d, sl in events:
                if k == EV_FRAME and a != 0xff:
                    m.frame = dict(type=a, flags=b & 0xff, size=d, seen=0, pad=None)
                    if a == HEADERS:
                        m.block = dict(stream=c, flags=(b & END_STREAM) | (2 if b & PRIORITY else 0) | (b >> 8 & 0xff) << 8, frag=bytearray())
                        if d < m._lo():
                            raise HpackError(ERR_PADDING)
                elif k == EV_PAYLOAD and m.frame is not None:
                    f = m.frame
                    if f["type"] in (HEADERS, CONTINUATION) and m.block is not None:
                        m._fragment(slices[sl][a:a + b])
                    f["seen"] += b
                    if c:
                        m.frame = None
                        if f["type"] in (HEADERS, CONTINUATION) and f["flags"] & END_HEADERS and m.block is not None:
                            closed.append(bytes(m.block["frag"]))
                            good = copy.deepcopy(m.table)
                            try:
                                decoded = m.table.decode_block(bytes(m.block["frag"]))
                            except HpackError:
                                m.table = good  # (the table behind the last good block)
                                raise
                            first = len(fields)
                            for name, value, rep in decoded:
                                fields.append((len(strings), len(strings) + len(name), len(name) | rep << 24, len(value)))
                                strings += name + value
                            blocks.append((m.block["stream"], first, len(fields) - first, m.block["flags"]))
                            m.block = None
        except HpackError as e:
            failure = FAILED | e.code << 8 | m.block["stream"] << 32
            m.frame = m.block = None
        m.word |= failure
        word = m.word | (OPEN if m.block is not None else 0)
        totals = (len(blocks), len(fields), len(strings), m.table.inserted - ins0, m.table.evicted - ev0, m.table.size, word)
        if len(blocks) > caps[0] or len(fields) > caps[1] or len(strings) > caps[2]:
            return [], [], b"", totals + (1,), True  # nothing written, nothing committed, not taken
        self.table, self.frame, self.block, self.word = m.table, m.frame, m.block, m.word
        st = self.stats
        st["calls"] += 1
        st["blocks"] += len(blocks)
        st["fields"] += len(fields)
        st["string_bytes"] += len(strings)
        st["inserted"] += totals[3]
        st["evicted"] += totals[4]
        st["flags"] = self.word
        return blocks, fields, bytes(strings), totals + (0,), False

    def _lo(self):
        f = self.frame
        return (1 if f["flags"] & PADDED else 0) + (5 if f["flags"] & PRIORITY else 0) if f["type"] == HEADERS else 0

    def _fragment(self, data):
        """a piece of the open frame's payload: what of it is header block fragment goes to the open block"""
        f, lo = self.frame, self._lo()
        pos = f["seen"]
        padded = f["type"] == HEADERS and f["flags"] & PADDED
        if padded and f["pad"] is None and data:  # (the pad length is the payload's first byte)
            f["pad"] = data[0]
            if f["pad"] >= f["size"] - lo:
                raise HpackError(ERR_PADDING)
        hi = f["size"] - (f["pad"] or 0)
        a, b = max(lo, pos), min(hi, pos + len(data))
        if b > a:
            self.block["frag"] += data[a - pos:b - pos]
            if len(self.block["frag"]) > self.max_block:
                raise HpackError(ERR_BLOCK_TOO_LARGE)
