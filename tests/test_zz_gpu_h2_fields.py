"""The three big-endian fields of the HTTP/2 kernels at the top of their range: the 24-bit frame length, the 31-bit
stream id and the 32-bit gRPC message length.  Every kernel here assembles or takes them apart byte by
byte, and the rest of the suite feeds them stream ids below 2^14, frames below 2^16 and messages below 2^24 -- a top byte
that is dropped goes unseen there.  The reference is the oracle throughout: pyorc.h2_frame_batch for framing,
pyorc.H2Parser for events; every comparison is exact.

Parity alone does not pin the deframer's fast paths: a boundary step or bulk step that misreads a field DECLINES, and the
byte-wise automaton behind it delivers the right events slowly.  So the fast-path cases also assert that the path was
taken, against counts from a plain-Python restatement of the two rules over the slice list alone (Witness below; the
counts never come from a device run or from the host build of grdma_h2_fast.h, which is the code under test).  The
counts are pinned per case and checked when this module is imported, GPU or not."""
import fcntl
import functools
import os

import pytest

from oracle import pyorc
from tests import h2_device_lib as links_mod
from tests.h2_asm_model import OK
from tests.h2_device_lib import (FH, FLOW_SIZES, SENTINEL, STEPPED, UNPADDED, RHarness, _interleaved, check_reply, device_bytes,
                                 oracle_feed, oracle_parser, pack_slices, read_slices, receiver_slices, same)
from tests.h2_helpers import frame

pytestmark = pytest.mark.gpu

# ---- the field values ------------------------------------------------------------------------------------------------
ID_A, ID_B, ID_C, ID_D, ID_E = 0x01020305, 0x7FFFFFFF, 0x00FF0001, 0x00010001, 0x7F000001
IDS = (ID_A, ID_B, ID_C, ID_D, ID_E)
F16M = (1 << 24) - 1                       # the largest frame: 0xffffff on the wire
L16M4, L16M7 = (1 << 24) + 4, (1 << 24) + 7  # message lengths with a non-zero top byte
ERR_INVALID, ERR_CAPACITY = "error 2", "error 5"   # (as GrdmaError words them)

_PAT = bytes((j * 13 + 7) % 251 for j in range(251 * 16))


def body(n, k=0):
    """n payload bytes of message k (a 251-periodic pattern, rotated by k)"""
    r = k % 251
    return ((_PAT[r:] + _PAT[:r]) * (n // len(_PAT) + 1))[:n] if n else b""


def _oracle_lib():
    """the oracle is compiled on first use; this module uses it at import, where several workers may collect at once"""
    os.makedirs(os.path.join(os.path.dirname(pyorc.ORACLE_SO)), exist_ok=True)
    with open(os.path.join(os.path.dirname(pyorc.ORACLE_SO), ".fields_build.lock"), "w") as f:
        fcntl.flock(f, fcntl.LOCK_EX)
        pyorc.lib()


def oracle_framing(table, max_frame):
    """table: [(length, stream id, flags)] -> (bodies, wire, slice lengths) of the oracle's framing"""
    bodies = [body(n, k) for k, (n, _, _) in enumerate(table)]
    wire, lens = pyorc.h2_frame_batch(bodies, [s for _, s, _ in table], [f for _, _, f in table], max_frame)
    return bodies, wire, lens


def cut(wire, lens):
    out, o = [], 0
    for n in lens:
        out.append(wire[o:o + n])
        o += n
    assert o == len(wire)
    return out


# ---- framer ------------------------------------------------------------------------------------------------------------
def _empties(l1, l2, l3):
    """runs of 1, 2 and 5 empty messages, each in front of a non-empty one: the leader of a run walks it and the
    message behind it (modes 2 and 0), the 23-byte inlined slice fills and splits"""
    return [(7, ID_A, 0), (0, ID_B, 0), (l1, ID_A, 1), (0, ID_A, 0), (0, ID_B, 2), (l2, ID_E, 0), (0, ID_C, 0),
            (0, ID_B, 1), (0, ID_A, 0), (0, ID_D, 2), (0, ID_E, 0), (l3, ID_B, 3), (9, ID_C, 0), (0, ID_D, 2)]


FRAME_CASES = {
    # the closed form (mode 1): non-empty behind non-empty, max_frame > 5
    "closed_f6": ([(1, ID_A, 0), (7, ID_B, 1), (30, ID_C, 2), (100, ID_E, 3), (6, ID_D, 0), (1, ID_A, 0)], 6),
    "closed_f65535": ([(70000, ID_A, 0), (65530, ID_B, 1), (65531, ID_E, 0), (200000, ID_A, 2), (7, ID_C, 1)], 65535),
    "closed_f65536": ([(70000, ID_B, 0), (65531, ID_A, 1), (65532, ID_D, 0), (262144, ID_E, 2), (7, ID_A, 1)], 65536),
    "closed_f1m": ([((1 << 20) + 100, ID_B, 0), ((3 << 20) - 5, ID_A, 1), (9, ID_E, 2)], 1 << 20),
    "closed_f16m_len16m4": ([(L16M4, ID_A, 2), (300, ID_B, 0)], F16M),
    "closed_f65536_len16m7": ([(L16M7, ID_E, 1), (5, ID_D, 0)], 65536),   # 257 frames: a lane writes five slots
    # the sequential walk behind runs of empty messages (modes 2 and 0)
    "empties_f6": (_empties(10, 30, 6), 6),
    "empties_f65535": (_empties(70000, 65530, 200000), 65535),
    "empties_f65536": (_empties(70000, 65531, 200000), 65536),
    "empties_f1m": (_empties((1 << 20) + 100, 5, 2 << 20), 1 << 20),
    "empties_f16m_len16m4": (_empties(300, L16M4, 7), F16M),
    "empties_f16384_len16m7": ([(0, ID_A, 0), (L16M7, ID_B, 2)], 16384),  # (max_frame <= 5 would be millions of frames)
    # the sequential walk at max_frame <= 5
    "walk_f5": ([(20, ID_A, 0), (0, ID_B, 0), (21, ID_E, 1), (22, ID_A, 0), (0, ID_C, 0), (0, ID_D, 0), (23, ID_B, 2),
                 (1, ID_A, 3)], 5),
}
for _name, (_t, _mf) in FRAME_CASES.items():
    assert any(s >= 1 << 24 for _, s, _ in _t), _name
    assert {s for _, s, _ in _t} <= set(IDS), _name
    assert any(5 + n >= _mf for n, _, _ in _t), _name + ": no full-size frame"
assert any(_mf >> 16 for _, _mf in FRAME_CASES.values())   # frames with a non-zero top length byte
assert {_mf for _, _mf in FRAME_CASES.values()} >= {5, 6, 65535, 65536, 1 << 20, F16M}


class Framing:
    """One table framed on the device: the payloads in one pool at odd offsets, slice table and header arena filled with
    a sentinel and with room behind the caps, the arena at byte `hdr_off` of its 16-byte block."""

    def __init__(self, g, table, max_frame, hdr_off=0):
        self.g, self.table, self.max_frame, self.hdr_off = g, table, max_frame, hdr_off
        self.bodies, self.wire, self.lens = oracle_framing(table, max_frame)
        pool, self.offs = bytearray(), []
        for k, b in enumerate(self.bodies):
            pool += b"\xee" * ((3 * k + 1) % 16)
            self.offs.append(len(pool))
            pool += b
        self.pool = g.DeviceBuffer(data=bytes(pool) + bytes(16))

    def run(self, slices_cap=None, hdr_cap=None, slack=4):
        """-> (slice count, wire bytes the call reported); raises GrdmaError as the call does"""
        from grpc_rdma_amd import h2dev
        n_exp = len(self.lens)
        self.cap = n_exp + slack if slices_cap is None else slices_cap
        self.hdr_cap = 32 * (n_exp + slack) if hdr_cap is None else hdr_cap
        self.slices = self.g.DeviceBuffer(data=bytes([SENTINEL]) * (16 * (n_exp + slack + 4)))
        self.hdr = self.g.DeviceBuffer(data=bytes([SENTINEL]) * (32 * (n_exp + slack + 4)), offset=self.hdr_off)
        assert (self.hdr.ptr & 15) == self.hdr_off
        msgs = [(self.pool.ptr + o, n, s, f) for o, (n, s, f) in zip(self.offs, self.table)]
        return h2dev.frame_messages(msgs, self.max_frame, self.slices.ptr, self.cap, self.hdr.ptr, self.hdr_cap)

    def check(self, n, wire_bytes):
        """slice lengths, gathered wire bytes and wire_bytes against the oracle; -> the slices [(ptr, len)]"""
        got = read_slices(self.g, self.slices, n)
        assert n == len(self.lens) and [ln for _, ln in got] == self.lens
        # (payload slices point into the pool: read the pool once instead of one copy per slice)
        pool, hdr = self.pool.read(), self.hdr.read()
        parts = []
        for p, ln in got:
            if self.pool.ptr <= p and p + ln <= self.pool.ptr + len(pool):
                parts.append(pool[p - self.pool.ptr:p - self.pool.ptr + ln])
            elif self.hdr.ptr <= p and p + ln <= self.hdr.ptr + len(hdr):
                parts.append(hdr[p - self.hdr.ptr:p - self.hdr.ptr + ln])
            else:
                parts.append(device_bytes(self.g, p, ln))
        wire = b"".join(parts)
        assert len(wire) == len(self.wire) == wire_bytes
        same(wire, self.wire, "wire")
        return got

    def arena_slices(self, got):
        return [(p, ln) for p, ln in got if self.hdr.ptr <= p < self.hdr.ptr + self.hdr_cap]


@pytest.mark.parametrize("case", sorted(FRAME_CASES))
def test_framer_ids_frames_and_lengths_in_every_layout(gpu, case):
    """Every value class through the closed form, the walk behind runs of 1, 2 and 5 empty messages and the walk at
    max_frame <= 5: slice lengths, gathered wire bytes and wire_bytes equal the oracle's."""
    table, max_frame = FRAME_CASES[case]
    f = Framing(gpu, table, max_frame)
    f.check(*f.run())


def test_framer_refuses_max_frame_zero_and_two_to_the_24(gpu):
    f = Framing(gpu, [(7, ID_A, 0)], 16384)
    for bad in (0, 1 << 24):
        f.max_frame = bad
        with pytest.raises(gpu.GrdmaError, match=ERR_INVALID):
            f.run()
    f.max_frame = F16M
    f.bodies, f.wire, f.lens = oracle_framing(f.table, F16M)
    f.check(*f.run())


# one-frame and many-frame messages (more than 64 frames: a lane writes several slots) and an empty run; first frames
# are 14-byte headers, later frames 9-byte headers
OFF_TABLE = [(100, ID_A, 0), (66 * 1000 + 3, ID_B, 1), (995, ID_E, 2), (0, ID_A, 0), (0, ID_C, 0), (5, ID_B, 0),
             (130 * 1000, ID_A, 3), (1, ID_D, 0)]


@pytest.mark.parametrize("hdr_off", [1, 8, 15])
def test_framer_header_arena_off_alignment(gpu, hdr_off):
    """The byte-store branch of h2_emit_message: the header arena at 1, 8 and 15 bytes past a 16-byte boundary."""
    f = Framing(gpu, OFF_TABLE, 1000, hdr_off=hdr_off)
    got = f.check(*f.run())
    arena = f.arena_slices(got)
    assert all((p - f.hdr.ptr) % 32 == 0 for p, _ in arena)
    # byte stores write the header and nothing else: the rest of every slot and the arena behind the slots are untouched
    hdr = f.hdr.read()
    for p, ln in arena:
        assert hdr[p - f.hdr.ptr + ln:p - f.hdr.ptr + 32] == bytes([SENTINEL]) * (32 - ln)
    assert hdr[32 * len(arena):] == bytes([SENTINEL]) * (len(hdr) - 32 * len(arena))


# lengths cycle through {0, 0, 1, 7, 30}: the runs of two empty messages sit at (5 k, 5 k + 1), so one crosses the
# 256-message pass of k_h2_frame_index at (255, 256) and the four-message workgroups of k_h2_frame_one at (15, 16);
# the 4096-message table ends inside a run and the one message more is the run's second
LAUNCH_LENS = [(0, 0, 1, 7, 30)[i % 5] for i in range(4097)]
assert LAUNCH_LENS[255] == LAUNCH_LENS[256] == 0 and LAUNCH_LENS[15] == LAUNCH_LENS[16] == 0
assert LAUNCH_LENS[4095] == LAUNCH_LENS[4096] == 0


def launch_table(n, lens=LAUNCH_LENS):
    return [(lens[i], 2 * i + 1 + (1 << 24), i % 4) for i in range(n)]


@pytest.mark.parametrize("n", [4096, 4097], ids=["one_launch", "two_launches"])
def test_framer_both_launch_forms_on_one_table(gpu, n):
    """k_h2_frame_one at its largest table and k_h2_frame_index + k_h2_frame_emit on the same table plus one message,
    max_frame 16, ids up to 2 x 4097 + 2^24."""
    f = Framing(gpu, launch_table(n), 16)
    f.check(*f.run())


CAP_TABLES = {
    "closed": ([(70000, ID_A, 0), (7, ID_B, 1), (200000, ID_E, 2), (65531, ID_C, 0)], 65536),
    "empties": (_empties(70000, 65531, 200000), 65536),
    "closed_two_launches": (launch_table(4097, [(3, 9, 1, 7, 30)[i % 5] for i in range(4097)]), 16),
    "empties_two_launches": (launch_table(4097), 16),
}


@pytest.mark.parametrize("case", sorted(CAP_TABLES))
def test_framer_exact_capacity_and_overflow(gpu, case):
    """Slice table and header arena exactly full succeed; one entry short returns GRDMA_ERR_CAPACITY and leaves every
    byte at or behind the cap as it was (the guards that keep the stores inside the arrays)."""
    table, max_frame = CAP_TABLES[case]
    f = Framing(gpu, table, max_frame)
    n_exp = len(f.lens)
    got = f.check(*f.run())
    arena = f.arena_slices(got)
    in_use = max(p - f.hdr.ptr for p, _ in arena) + 32
    # a consistency check of the layout, not a comparison with the oracle: one 32-byte slot per inlined slice, packed
    assert in_use % 32 == 0 and in_use <= 32 * n_exp and in_use == 32 * len(arena)
    sent = bytes([SENTINEL])
    # the slice table exactly full / one entry short
    f.check(*f.run(slices_cap=n_exp))
    assert f.slices.read(off=16 * n_exp) == sent * (f.slices.nbytes - 16 * n_exp)
    with pytest.raises(gpu.GrdmaError, match=ERR_CAPACITY):
        f.run(slices_cap=n_exp - 1)
    assert f.slices.read(off=16 * (n_exp - 1)) == sent * (f.slices.nbytes - 16 * (n_exp - 1))
    # the arena exactly full / one slot short / one byte short
    f.check(*f.run(hdr_cap=in_use))
    assert f.hdr.read(off=in_use) == sent * (f.hdr.nbytes - in_use)
    for short in (in_use - 32, in_use - 1):
        with pytest.raises(gpu.GrdmaError, match=ERR_CAPACITY):
            f.run(hdr_cap=short)
        assert f.hdr.read(off=short) == sent * (f.hdr.nbytes - short)
        assert f.slices.read(off=16 * f.cap) == sent * (f.slices.nbytes - 16 * f.cap)


# ---- the witness: which message starts the boundary step takes, which frames the bulk step takes ---------------------
def boundary_rule(s, next_len, sid, need, max_frame):
    """The boundary step's rule (the comments of csrc/grdma_h2_fast.h) for slice s of stream `sid`, of whose open
    message `need` bytes are still to come (0: at a message header): the slice holds at most one closing DATA frame of
    1..9 payload bytes that finishes the open message, then a DATA header of the same stream with flags 0, then the
    5-byte header of a non-empty message that the frame does not outlive, and the frame ends with this slice or exactly
    with the next.  -> (slices taken, message bytes still to come) or None."""
    o = 0
    if need:
        if not 1 <= need <= 9 or len(s) < 9 + need + 14 or s[:9] != frame(0, 0, sid, bytes(need))[:9]:
            return None
        o = 9 + need
    elif len(s) < 14:
        return None
    fs, mlen = int.from_bytes(s[o:o + 3], "big"), int.from_bytes(s[o + 10:o + 14], "big")
    if s[o + 3:o + 5] != b"\0\0" or int.from_bytes(s[o + 5:o + 9], "big") & 0x7FFFFFFF != sid or not 5 <= fs <= max_frame:
        return None
    if s[o + 9] > 1 or mlen == 0 or mlen + 5 < fs:
        return None
    avail = len(s) - o - 9
    if avail > fs or (fs > avail and next_len != fs - avail):
        return None
    return (2 if fs > avail else 1), mlen - (fs - 5)


def bulk_rule(s, next_len, sid, need, max_frame):
    """The bulk step's rule (csrc/grdma_h2_kernels.h, "bulk step"): behind a message's first frame, a DATA frame of the
    stream that is mid-message, flags 0, inside the message, in exactly two slices -- 9 + p0 bytes, then p1 > 0 bytes.
    -> the frame's size or None."""
    if need == 0 or len(s) < 9 or next_len is None:
        return None
    fs = int.from_bytes(s[:3], "big")
    if s[3:5] != b"\0\0" or int.from_bytes(s[5:9], "big") & 0x7FFFFFFF != sid or fs > max_frame or fs > need:
        return None
    p0 = len(s) - 9
    return fs if p0 < fs and next_len == fs - p0 else None


class Witness:
    """A sequential walk of one deframe call over HEADERS (END_HEADERS) and DATA frames: where a slice starts at a frame
    header and the stream of the last frame is still the current one, the two rules are asked; everything else goes byte
    range by byte range.  Knows nothing of events."""

    def __init__(self, open_ids, max_frame, boundary=True):
        self.max_frame, self.boundary = max_frame, boundary
        self.need = {s: 0 for s in open_ids}   # message bytes still to come
        self.mh = {s: b"" for s in open_ids}   # a message header met in pieces
        self.read_closed = set()
        self.cur = None                        # the stream of the last frame that named one (none at the call's start)
        self.fh, self.left, self.in_frame = b"", 0, False
        self.data, self.flags, self.sid = False, 0, 0
        self.steps = self.frames = 0

    def run(self, slices):
        i = 0
        while i < len(slices):
            s = slices[i]
            nxt = len(slices[i + 1]) if i + 1 < len(slices) else None
            c = self.cur
            if not self.in_frame and not self.fh and c is not None and c not in self.read_closed and not self.mh[c]:
                m = boundary_rule(s, nxt, c, self.need[c], self.max_frame) if self.boundary else None
                if m:
                    self.steps += 1
                    self.need[c] = m[1]
                    i += m[0]
                    continue
                fs = bulk_rule(s, nxt, c, self.need[c], self.max_frame)
                if fs:
                    self.frames += 1
                    self.need[c] -= fs
                    i += 2
                    continue
            self.feed(s)
            i += 1
        return self.steps, self.frames

    def feed(self, s):
        pos = 0
        while pos < len(s):
            if not self.in_frame:
                take = min(9 - len(self.fh), len(s) - pos)
                self.fh += s[pos:pos + take]
                pos += take
                if len(self.fh) == 9:
                    h, self.fh = self.fh, b""
                    self.left, ftype, self.flags = int.from_bytes(h[:3], "big"), h[3], h[4]
                    self.sid = int.from_bytes(h[5:9], "big") & 0x7FFFFFFF
                    assert ftype == 0 or (ftype == 1 and self.flags == 4), "the walk knows HEADERS | END_HEADERS and DATA"
                    self.cur = self.sid if self.sid in self.need else None
                    self.data = ftype == 0 and self.cur is not None and self.sid not in self.read_closed
                    self.in_frame = True
                    if self.left == 0:
                        self.end_frame()
            else:
                take = min(self.left, len(s) - pos)
                if self.data:
                    self.message_bytes(s[pos:pos + take])
                pos += take
                self.left -= take
                if self.left == 0:
                    self.end_frame()

    def message_bytes(self, b):
        sid, pos = self.sid, 0
        while pos < len(b):
            if self.need[sid] == 0:
                take = min(5 - len(self.mh[sid]), len(b) - pos)
                self.mh[sid] += b[pos:pos + take]
                pos += take
                if len(self.mh[sid]) == 5:
                    self.need[sid], self.mh[sid] = int.from_bytes(self.mh[sid][1:], "big"), b""
            else:
                take = min(self.need[sid], len(b) - pos)
                self.need[sid] -= take
                pos += take

    def end_frame(self):
        self.in_frame = False
        if self.data and self.flags & 1:
            self.read_closed.add(self.sid)


SMALL_MSGS = [(7, ID_B, 0), (30, ID_B, 1), (1, ID_B, 0), (0, ID_A, 0), (12, ID_A, 0), (6, ID_A, 0), (2, ID_E, 2)]
# name -> (messages [(length, stream id, flags)], max_frame, {shape: (boundary steps, bulk frames, bulk frames with the
# boundary step off)}): what the predicate gives, pinned; the claims the names make are asserted below
DEFRAME_CASES = {
    # one stream with four distinct id bytes, frames of 0x010000: six message starts, all of them the step's in both
    # shapes (closing frames of 0, 1, 9 and thousands of bytes; the 7-byte message is its own frame)
    "id01020305_f65536": ([(70000, ID_A, 0), (65532, ID_A, 0), (131076, ID_A, 0), (196603, ID_A, 0), (65540, ID_A, 1),
                           (65536 + 4, ID_A, 0)], 65536),
    "id7fffffff_f131072": ([(131072 * 2, ID_B, 0), (131068, ID_B, 0), (131072 + 4, ID_B, 1), (300000, ID_B, 0),
                            (131072 - 5 + 1, ID_B, 0), (262144 + 4, ID_B, 0)], 131072),
    # five ids on one connection, an empty message between big ones, END_STREAM on a big id
    "five_ids_f65535": ([(70000, ID_A, 0), (131069, ID_A, 0), (65535 + 4, ID_C, 0), (70000, ID_C, 1), (0, ID_C, 0),
                         (131074, ID_C, 0), (65531, ID_E, 0), (200000, ID_E, 0), (65535 * 2 - 5, ID_D, 0), (9, ID_D, 2),
                         (65530, ID_B, 0), (65539, ID_B, 2)], 65535),
    "five_ids_f1m": ([((1 << 20) + 4, ID_E, 0), (3 << 20, ID_E, 0), ((2 << 20) - 5, ID_A, 0), (0, ID_A, 0),
                      ((1 << 20) + 100, ID_A, 1), ((1 << 20) - 4, ID_B, 0), (40, ID_B, 2)], 1 << 20),
    # the switch of h2_msg_plain: the framer's layouts at max_frame 6 and 5, frames of a few bytes
    "three_ids_f6": (SMALL_MSGS, 6),
    "three_ids_f5": (SMALL_MSGS, 5),
    # message lengths with a non-zero top byte: 2^24 + 4 leaves a 9-byte closing frame at 1 MiB frames and reaches the
    # step's edge; 2^24 + 7 leaves 12 bytes, so the receiver's second start is correctly not the step's
    "len16m4_f1m": ([(L16M4, ID_B, 0), (L16M4, ID_B, 1)], 1 << 20),
    "len16m7_f1m": ([(L16M7, ID_A, 0), (L16M7, ID_A, 0)], 1 << 20),
    # ... at 16 KiB frames: 1025 frames, 1024 of them the bulk step's in sixteen steps or more; the closing frame has
    # 12 bytes
    "len16m7_f16384": ([(L16M7, ID_B, 1), (5, ID_B, 0)], 16384),
    # ... and in frames of 0xffffff, END_STREAM on the last
    "len16m_f16m": ([(L16M4, ID_E, 0), (L16M7, ID_E, 2)], F16M),
}
WITNESS = {
    "id01020305_f65536": {"sender": (6, 8, 8), "receiver": (6, 4, 4)},
    "id7fffffff_f131072": {"sender": (6, 9, 9), "receiver": (6, 4, 4)},
    "five_ids_f65535": {"sender": (4, 12, 12), "receiver": (4, 8, 8)},
    "five_ids_f1m": {"sender": (1, 7, 7), "receiver": (1, 3, 3)},
    "three_ids_f6": {"sender": (4, 9, 9), "receiver": (0, 0, 0)},
    "three_ids_f5": {"sender": (0, 9, 9), "receiver": (0, 0, 0)},
    "len16m4_f1m": {"sender": (2, 32, 32), "receiver": (2, 30, 30)},
    "len16m7_f1m": {"sender": (2, 32, 32), "receiver": (1, 30, 30)},
    "len16m7_f16384": {"sender": (2, 1024, 1024), "receiver": (1, 1023, 1023)},
    "len16m_f16m": {"sender": (2, 1, 1), "receiver": (1, 0, 0)},
}
SHAPES = ("sender", "receiver")


def streams_of(msgs):
    return sorted({s for _, s, _ in msgs})


def slice_list(case, shape):
    """HEADERS (END_HEADERS) for every stream, then the oracle's own framing of the case's messages: its slice list
    (sender) or the endpoint reads of it (receiver)"""
    msgs, max_frame = DEFRAME_CASES[case]
    _, wire, lens = oracle_framing(msgs, max_frame)
    tx = cut(wire, lens)
    return [frame(1, 4, s, b"\x82") for s in streams_of(msgs)] + (tx if shape == "sender" else receiver_slices(tx))


def witness_counts(case, shape):
    msgs, max_frame = DEFRAME_CASES[case]
    sl = slice_list(case, shape)
    on = Witness(streams_of(msgs), max_frame, True).run(sl)
    off = Witness(streams_of(msgs), max_frame, False).run(sl)
    assert off[0] == 0
    return on + (off[1],)


def _check_witness():
    _oracle_lib()
    for case in DEFRAME_CASES:
        for shape in SHAPES:
            got = witness_counts(case, shape)
            assert WITNESS[case][shape] == got, "%s %s: the predicate gives %r" % (case, shape, got)
    # what the names claim: every message start of the one-stream cases is the step's, in both shapes; 2^24 + 4 at
    # 1 MiB frames reaches the step's edge in both shapes, 2^24 + 7 misses it on the receiving side; every case has
    # frames for the bulk step, and the step has message starts at every frame size above 5
    for case in ("id01020305_f65536", "id7fffffff_f131072", "len16m4_f1m"):
        assert all(WITNESS[case][sh][0] == len(DEFRAME_CASES[case][0]) for sh in SHAPES), case
    assert [WITNESS["len16m7_f1m"][sh][0] for sh in SHAPES] == [2, 1]
    assert all(WITNESS[case]["sender"][1] > 0 for case in DEFRAME_CASES if case != "len16m_f16m")
    assert all(WITNESS[case]["sender"][0] > 0 for case in DEFRAME_CASES if DEFRAME_CASES[case][1] > 5)
    assert all(any(s >= 1 << 24 for _, s, _ in DEFRAME_CASES[case][0]) for case in DEFRAME_CASES)


_check_witness()


# ---- deframer ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def deframe_case(case, shape):
    """-> (slices, the oracle's events for them)"""
    msgs, max_frame = DEFRAME_CASES[case]
    sl = slice_list(case, shape)
    return sl, expected_events(sl, streams_of(msgs), max_frame)


def expected_events(slices, ids, max_frame, parser=None):
    p = parser or oracle_parser(False, max_frame, ids)
    # (the default cap is two events per byte: gigabytes at 16 MiB)
    rc, ev = oracle_feed(p, slices, cap=lambda s: min(2 * len(s) + 64, 4096))
    assert rc == 0
    return ev


def pack(slices, odd):
    """the slices in one arena, 16-byte packed or at odd offsets with filler between them -> (arena, [(offset, len)])"""
    return pack_slices(slices, STEPPED if odd else UNPADDED)


def device_events(g, buf, table, ids, max_frame, cap, **kw):
    """-> (events, boundary steps, frames parsed in bulk steps) of one call on a fresh parser"""
    from grpc_rdma_amd import h2dev
    p = h2dev.Parser(False, max_frame, chunks=False, **kw)
    assert p.open_streams(ids) == 0
    err, ev = p.deframe(buf.ptr, table, cap=cap)
    steps, frames = p.last_boundary_steps, p.last_bulk_frames
    p.close()
    assert err == 0
    return ev, steps, frames


def assert_events(got, exp):
    same(got, exp, "events")


PACKINGS = [False, True]
PACK_IDS = ["packed", "odd_offsets"]


@pytest.mark.parametrize("odd", PACKINGS, ids=PACK_IDS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", sorted(DEFRAME_CASES))
def test_deframe_parity_on_every_path(gpu, case, shape, odd):
    """The oracle's events with the boundary step on and off, 64 and 32 frames per bulk step; ids whose home slot in
    the stream table is far from slot 0 (tab_home of 0x7fffffff is the table's last slot: the probe wraps)."""
    msgs, max_frame = DEFRAME_CASES[case]
    sl, exp = deframe_case(case, shape)
    arena, table = pack(sl, odd)
    buf = gpu.DeviceBuffer(data=arena)
    for boundary in (True, False):
        for pairs in (True, False):
            ev, steps, _ = device_events(gpu, buf, table, streams_of(msgs), max_frame, len(exp) + 64,
                                         boundary_step=boundary, bulk_pairs=pairs)
            assert_events(ev, exp)
            assert boundary or steps == 0
    buf.free()


@pytest.mark.parametrize("odd", PACKINGS, ids=PACK_IDS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", sorted(DEFRAME_CASES))
def test_deframe_fast_paths_are_taken(gpu, case, shape, odd):
    """last_boundary_steps and bulk_frames equal the counts the Witness predicate gives for the slice list: a step that
    drops a byte of a field declines, the events stay right, and only these counts show it."""
    msgs, max_frame = DEFRAME_CASES[case]
    sl, exp = deframe_case(case, shape)
    w_steps, w_frames, w_frames_off = WITNESS[case][shape]
    arena, table = pack(sl, odd)
    buf = gpu.DeviceBuffer(data=arena)
    for pairs in (True, False):
        ev, steps, frames = device_events(gpu, buf, table, streams_of(msgs), max_frame, len(exp) + 64,
                                          boundary_step=True, bulk_pairs=pairs)
        print("%s %s pairs=%d: boundary steps %d (witness %d), bulk frames %d (witness %d)" %
              (case, shape, pairs, steps, w_steps, frames, w_frames))
        assert_events(ev, exp)
        assert (steps, frames) == (w_steps, w_frames)
        ev, steps, frames = device_events(gpu, buf, table, streams_of(msgs), max_frame, len(exp) + 64,
                                          boundary_step=False, bulk_pairs=pairs)
        assert (steps, frames) == (0, w_frames_off)
    buf.free()


# 840 messages in 2100 slices: the chunked deframer plans a list of >= 2048; frames of 0x010000 and 0x000001 on the wire
CHUNK_LENS = [(300, 9, 65532, 5)[i % 4] for i in range(840)]


@pytest.mark.parametrize("odd", PACKINGS, ids=PACK_IDS)
def test_deframe_chunked_and_merged(gpu, odd):
    """The chunked deframer (k_h2_deframe_chunks / k_h2_merge_or_deframe) at id 0x7fffffff and 64 KiB frames: the first
    call leaves the boundary step's hint, the long list is planned, verified and merged, the events are the oracle's
    and the call behind it finds the state the merge installed."""
    from grpc_rdma_amd import h2dev
    max_frame = 65536
    p = h2dev.Parser(False, max_frame, boundary_step=True)
    o = pyorc.H2Parser(expect_client_prefix=False, max_frame_size=max_frame)
    assert p.open_streams([ID_A, ID_B]) == 0 and o.open_stream(ID_A) == 0 and o.open_stream(ID_B) == 0
    calls = [[(70000, ID_B, 0)] * 3, [(n, ID_B, 0) for n in CHUNK_LENS], [(7, ID_B, 0), (131076, ID_B, 0), (9, ID_A, 2)]]
    for k, msgs in enumerate(calls):
        _, wire, lens = oracle_framing(msgs, max_frame)
        sl = ([frame(1, 4, ID_B, b"\x82")] if k == 0 else []) + cut(wire, lens)
        assert k != 1 or len(sl) >= 2048
        exp = expected_events(sl, (), max_frame, parser=o)
        arena, table = pack(sl, odd)
        buf = gpu.DeviceBuffer(data=arena)
        err, ev = p.deframe(buf.ptr, table, cap=8 * len(sl) + 4096)
        assert err == 0
        assert_events(ev, exp)
        assert p.chunk_stats() == ((0, 0) if k == 0 else (1, 1))
        buf.free()
    p.close()


# ---- the chains behind the deframer ------------------------------------------------------------------------------------
CHAIN_MSGS = [(70000, ID_A, 0), (0, ID_B, 1), (200000, ID_B, 0), (300, ID_E, 1), (65531, ID_A, 0), (1, ID_C, 0)]
assert ID_B >= 1 << 30 and ID_E >= 1 << 30


def _chain_feed(g, max_frame=65536):
    """the chain's messages framed by the oracle at 64 KiB frames, fed to a device parser + assembler and the model"""
    bodies, wire, lens = oracle_framing(CHAIN_MSGS, max_frame)
    h = RHarness(g, 1 << 20, streams=streams_of(CHAIN_MSGS), max_frame=max_frame)
    got = h.feed(receiver_slices(cut(wire, lens)))   # (compares every descriptor with tests/h2_asm_model.py and the bytes)
    return h, got, bodies


def test_assembler_descriptors_carry_the_id_and_length(gpu):
    h, got, bodies = _chain_feed(gpu)
    assert [(m.stream_id, m.length, m.flags, m.status) for m in got] == [(s, n, f & 1, OK) for n, s, f in CHAIN_MSGS]
    assert [h.asm.view(m) for m in got] == bodies
    h.close()


ROUTES = {ID_A: ID_B, ID_B: ID_A, ID_E: ID_C, ID_C: 0x7F0000FF}


def test_reply_on_big_ids_at_64k_frames(gpu):
    """k_h2_reply_plan / k_h2_reply_emit: routed replies whose targets are big ids, reply frames of 0x010000: slice
    lengths and wire against h2_frame_batch, as check_reply compares them."""
    from grpc_rdma_amd import h2dev
    h, got, bodies = _chain_feed(gpu)
    reply = h2dev.Reply(h.asm, list(ROUTES.items()), 65536, 64)
    _, wire = check_reply(gpu, h, reply, 65536, ROUTES)
    assert all(frame(0, 0, ROUTES[s])[5:9] in wire for _, s, _ in CHAIN_MSGS)
    reply.close()
    h.close()


def test_window_updates_carry_the_four_id_bytes(gpu):
    """k_h2_fc_emit: WINDOW_UPDATE frames for big-id streams, against the model of tests/h2_flow_model.py (FH.feed
    compares slices, wire and counters exactly)."""
    ids = (ID_A, ID_B, ID_E, ID_C)
    h = FH(gpu, streams=ids, stream_window=1 << 20, conn_window=1 << 24, conn_threshold=0)
    res, wire = h.feed(_interleaved(0, ids, FLOW_SIZES))
    assert res[0] == 5 and res[5] == 0
    assert sorted(s for s, _ in h.model.frames) == sorted((0,) + ids)
    assert [wire[13 * k + 5:13 * k + 9] for k in range(5)] == [s.to_bytes(4, "big") for s, _ in h.model.frames]
    res, _ = h.feed(_interleaved(1, ids, FLOW_SIZES[:6]))
    assert res[5] == 0
    h.close()


BIG_OF = {1: ID_A, 3: ID_B, 5: ID_E, 7: ID_C, 9: 0x40000001, 2: 0x01020304, 4: 0x7FFFFFFE}


def test_group_pipe_step_on_big_ids(gpu, monkeypatch):
    """k_h2_frame_links and k_h2_deframe_links share the bodies above: one step of the four-link group pipe of
    tests/h2_device_lib.py (Links) with the tables' stream ids replaced by big ones; slice tables, wire, delivered
    bytes and events per link against the oracle."""
    from grpc_rdma_amd import h2dev
    monkeypatch.setenv("GRDMA_H2_PIPE_FUSED", "1")
    monkeypatch.setattr(links_mod, "TABLES", [[(n, BIG_OF[s], f) for n, s, f in t] for t in links_mod.TABLES])
    L = links_mod.Links(gpu)
    parsers = [L.parser(li) for li in range(4)]
    gp = h2dev.GroupPipe(L.job, [L.spec(li, parsers[li][0]) for li in range(4)])
    links_mod._check_steps(L, gp, [0, 1, 2, 3], parsers, 1)
    assert all(frame(0, 0, s)[5:9] in L.wire[li] for li in range(4) for _, s, _ in links_mod.TABLES[li])
    gp.close()
    for p, _ in parsers:
        p.close()
    L.close()
