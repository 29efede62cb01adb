"""The sequential reference of the call table (grdma_h2_calls, include/grdma_amd.h "Call table"): it defines the exact
output of a step.  Plain Python over tuples, no device and no numpy.

Inputs of a step, all lists of tuples in the layout of the C structs:
  blocks  (stream, first_field, nfields, flags)            grdma_h2_header_block; only flags bits 8..15 are read
  meta    the twelve words of grdma_h2_call_meta           record k belongs to block k
  msgs    (offset, length, seq, stream, status, flags)     grdma_h2_rx_msg
  events  (kind, a, b, c, d, slice)                        grdma_h2_event; only STREAM_CLOSED is read
Outputs: dispatch records (offset, length, call, stream, msg, method, word, seq, 0), the nmethods + 2 segment words, done
records (call, bytes, stream, method, messages, word), the eight result words and None, "capacity" or "invalid"."""
import struct

NONE = 0xffffffff
U64 = (1 << 64) - 1
REQUEST, VERDICT_OK, HAS_TIMEOUT = 1, 0, 1
STREAM_CLOSED = 7
FIRST, LAST, COMPRESSED = 1, 2, 4
NO_CALL, EXPIRED_MSG, BAD_STATUS, COMPRESSED_IDENTITY = 1, 2, 3, 4
READS_CLOSED, LEFT, DEADLINE = 1, 2, 3
WAS_READS_CLOSED = 1
E_READS_CLOSED, E_EXPIRED = 1, 2  # an entry's flags
BAD_INPUT, LOST = 1, 2            # result word 6
ERR_STREAM, ERR_METHOD = 1, 2
MAX_MSGS = 1 << 20
RESULT = ("opened", "dispatched", "orphans", "done", "expired", "live", "flags", "overflow")
STATS = ("steps", "opened", "messages", "bytes", "orphans", "done", "lost")


class Entry:
    __slots__ = ("call", "deadline", "bytes", "stream", "method", "messages", "encoding", "flags")

    def row(self):
        return (self.call, self.deadline, self.bytes, self.stream, self.method, self.messages, self.encoding | self.flags << 8)


def would_open(block, rec):
    """the first three conditions of OPEN: a REQUEST, verdict OK, status byte of the block 0"""
    return rec[1] & 0xff == REQUEST and rec[1] >> 8 & 0xff == VERDICT_OK and block[3] >> 8 & 0xff == 0


class CallsModel:
    def __init__(self, table_slots=0, nmethods=0):
        self.slots = table_slots or 4096
        assert self.slots >= 16 and self.slots & (self.slots - 1) == 0 and self.slots <= 65536 and 0 <= nmethods <= 4096
        self.nmethods = nmethods
        self.table = {}  # stream -> Entry
        self.serial = 0
        self.lost = 0
        self.stats = dict.fromkeys(STATS, 0)

    def dump(self):
        return [self.table[s].row() for s in sorted(self.table)]

    def step(self, blocks, meta, msgs, events, now, dispatch_cap, done_cap):
        assert len(blocks) == len(meta)
        nm = self.nmethods
        # bad input: the first record that would open a call and cannot name one
        for k, (b, r) in enumerate(zip(blocks, meta)):
            if would_open(b, r):
                code = ERR_STREAM if r[0] == 0 or r[0] >> 31 else ERR_METHOD if r[2] >= nm else 0
                if code:
                    return [], None, [], (0, 0, 0, 0, 0, 0, BAD_INPUT | code << 8 | k << 32, 0), "invalid"
        table = {s: self._copy(e) for s, e in self.table.items()}
        serial, lost, seen, opened = self.serial, self.lost, set(), 0
        # 1. OPEN
        for b, r in zip(blocks, meta):
            if not would_open(b, r):
                continue  # (refused or ignored)
            s = r[0]
            if s in self.table or s in seen:
                continue  # (duplicate: the first of the step wins, whether it opened or was lost)
            seen.add(s)
            if len(table) + 1 > self.slots // 2:
                lost = 1
                continue
            e = Entry()
            e.call, e.stream, e.method, e.encoding, e.flags, e.messages, e.bytes = serial, s, r[2], r[1] >> 16 & 0xff, 0, 0, 0
            e.deadline = min(U64, now + (r[5] | r[6] << 32)) if r[1] >> 24 & HAS_TIMEOUT else U64
            serial += 1
            opened += 1
            table[s] = e
        # 2. EXPIRE
        done = []
        for s in sorted(table):
            e = table[s]
            if not e.flags & E_EXPIRED and e.deadline <= now:
                e.flags |= E_EXPIRED
                done.append((e.call, e.bytes, s, e.method, e.messages, DEADLINE | (WAS_READS_CLOSED if e.flags & E_READS_CLOSED else 0) << 8))
        expired = len(done)
        # 3. MESSAGES
        closing = {ev[3] for ev in events if ev[0] == STREAM_CLOSED and ev[1] in (0, 1)}
        recs, d_bytes = [], 0
        for i, (off, length, _seq, s, status, flags) in enumerate(msgs):
            comp = COMPRESSED if flags & 1 else 0
            e = table.get(s)
            if status != 0:
                recs.append([nm, (off, length, 0, s, i, NONE, comp | BAD_STATUS << 8, 0, 0), None])
            elif e is None:
                recs.append([nm, (off, length, 0, s, i, NONE, comp | NO_CALL << 8, 0, 0), None])
            elif e.flags & E_EXPIRED:
                recs.append([nm, (off, length, e.call, s, i, NONE, comp | EXPIRED_MSG << 8 | e.encoding << 16, 0, 0), None])
            elif comp and e.encoding == 0:
                recs.append([nm, (off, length, e.call, s, i, NONE, comp | COMPRESSED_IDENTITY << 8, 0, 0), None])
            else:
                word = comp | (FIRST if e.messages == 0 else 0) | e.encoding << 16
                recs.append([e.method, (off, length, e.call, s, i, e.method, word, e.messages, 0), s])
                e.messages += 1
                e.bytes += length
                d_bytes += length
        # LAST: the last DISPATCHED message of its stream in the step, when the step holds a close of the stream
        last = {}
        for j, (_m, _r, s) in enumerate(recs):
            if s is not None:
                last[s] = j
        for s, j in last.items():
            if s in closing:
                r = recs[j][1]
                recs[j][1] = r[:6] + (r[6] | LAST,) + r[7:]
        # 4. CLOSE
        for ev in events:
            if ev[0] != STREAM_CLOSED or ev[3] not in table:
                continue
            e = table[ev[3]]
            if ev[1] == 0:
                e.flags |= E_READS_CLOSED
                done.append((e.call, e.bytes, e.stream, e.method, e.messages, READS_CLOSED))
            elif ev[1] == 1:
                done.append((e.call, e.bytes, e.stream, e.method, e.messages, LEFT | (WAS_READS_CLOSED if e.flags & E_READS_CLOSED else 0) << 8))
                del table[ev[3]]
        # the dispatch table: by method, stable; the orphans behind the last method
        order = sorted(range(len(recs)), key=lambda j: recs[j][0])
        dispatch = [recs[j][1] for j in order]
        counts = [0] * (nm + 1)
        for m, _r, _s in recs:
            counts[m] += 1
        segments = [0]
        for c in counts:
            segments.append(segments[-1] + c)
        orphans = counts[nm]
        res = (opened, len(recs) - orphans, orphans, len(done), expired, len(table), LOST if lost else 0, 0)
        if dispatch_cap < len(msgs) or done_cap < len(done):
            return [], None, [], res[:7] + (1,), "capacity"
        self.table, self.serial, self.lost = table, serial, lost
        st = self.stats
        st["steps"] += 1
        st["opened"] += opened
        st["messages"] += len(recs) - orphans
        st["bytes"] += d_bytes
        st["orphans"] += orphans
        st["done"] += len(done)
        st["lost"] = LOST if lost else 0
        return dispatch, segments, done, res, None

    @staticmethod
    def _copy(e):
        c = Entry()
        for k in Entry.__slots__:
            setattr(c, k, getattr(e, k))
        return c


# ---- the records' bytes -----------------------------------------------------------------------------------------------------
def dispatch_bytes(r):
    return struct.pack("<QQQIIIIII", *r)  # 48


def done_bytes(r):
    return struct.pack("<QQIIII", *r)  # 32


def entry_bytes(r):
    return struct.pack("<QQQIIIIII", *r, 0, 0)  # 48


# ---- rows for the inputs -----------------------------------------------------------------------------------------------------
def request(stream, method=0, timeout=None, encoding=0, verdict=0, kind=REQUEST, status=0):
    """(block, call record) of one header block"""
    flags = HAS_TIMEOUT if timeout is not None else 0
    t = timeout or 0
    word = kind | verdict << 8 | encoding << 16 | flags << 24
    return (stream, 0, 0, status << 8), (stream, word, method, NONE, NONE, t & NONE, t >> 32, NONE, NONE, NONE, 0, NONE)


def message(stream, length=8, offset=0, status=0, compressed=False, seq=0):
    return (offset, length, seq, stream, status, 1 if compressed else 0)


def closed(stream, left):
    return (STREAM_CLOSED, 1 if left else 0, 0, stream, 0, 0)
