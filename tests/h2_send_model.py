"""A sequential model of send flow control on the device (grdma_h2_sw, csrc/grdma_h2_sw.h): the rules of
include/grdma_amd.h ("Send flow control") applied to the ORACLE's event list (oracle/pyorc.H2Parser.feed) plus the bytes
that were fed, the grant as the sequential rule of DataSendContext::max_outgoing, and the wire as the oracle's
frame_one / sb_add (oracle/grdma_oracle.c) started at an offset.  Which streams the transport's map holds is read from
the oracle's parser.  Nothing of the library's own events or output goes into it; tests/test_h2_send_model.py pins it
against the oracle's framer and parser before a device test trusts it."""
import struct

from oracle.pyorc import EV_FRAME, EV_PAYLOAD

MAXW = (1 << 31) - 1
BAD_INCREMENT, WINDOW_OVERFLOW, BAD_SETTINGS, LOST = 1, 2, 4, 8  # GRDMA_H2_SW_*
STALL_CONN, STALL_STREAM, STALL_UNKNOWN = 1, 2, 4
INLINED = 23


def live_of(orc):
    """the stream ids the oracle's parser holds in its map"""
    return {int(orc.p.streams[i].stream_id) for i in range(int(orc.p.nstreams))}


# ---- the grant -------------------------------------------------------------------------------------------------------
def grant_sequential(rem, streams, windows, conn):
    """in table order each message gets min(remaining, its stream's window, the connection's window), and nothing once
    an earlier message of its stream is unfinished.  windows: stream -> window (may be negative), None = unknown"""
    w, blocked, out = dict(windows), set(), []
    for r, s in zip(rem, streams):
        if w.get(s) is None:
            out.append(0)
            continue
        g = 0 if s in blocked else max(0, min(r, w[s], conn))
        if g < r:
            blocked.add(s)
        w[s] -= g
        conn -= g
        out.append(g)
    return out


def grant_prefix(rem, streams, windows, conn):
    """the same in two prefix sums -> (a, g): a_i = min(r_i, max(0, W_s - sum of r_j over earlier messages of s)),
    g_i = min(a_i, max(0, C - sum of a_j over earlier messages))"""
    before, a = {}, []
    for r, s in zip(rem, streams):
        W = windows.get(s)
        a.append(0 if W is None else min(r, max(0, W - before.get(s, 0))))
        before[s] = before.get(s, 0) + r
    g, pre = [], 0
    for x in a:
        g.append(min(x, max(0, conn - pre)))
        pre += x
    return a, g


# ---- the wire: frame_one / sb_add of the oracle, started at an offset ---------------------------------------------------
def sb_add(sb, n, inl):
    """grpc_slice_buffer_add; sb: [[length, inlined], ...]"""
    if inl and sb and sb[-1][1] and sb[-1][0] < INLINED:
        if n + sb[-1][0] <= INLINED:
            sb[-1][0] += n
        else:
            cp = INLINED - sb[-1][0]
            sb[-1][0] = INLINED
            sb.append([n - cp, 1])
        return
    sb.append([n, inl])


def frame_piece(sb, wire, body, sid, flags, mf, p, g):
    """bytes [p, p + g) of [5-byte header | body] as DATA frames of at most mf bytes onto the outbuf sb / wire"""
    full = bytes([flags & 1]) + len(body).to_bytes(4, "big") + bytes(body)
    fcb = []
    if p < 5:
        fcb.append([5 - p, 1])
    if len(full) - max(p, 5) > 0:
        fcb.append([len(full) - max(p, 5), 0])
    fcb_len, off, left = len(full) - p, p, g
    while left > 0:
        send = min(left, mf)
        last = 1 if (flags & 2) and send == fcb_len else 0
        wire += send.to_bytes(3, "big") + bytes([0, last]) + sid.to_bytes(4, "big") + full[off:off + send]
        sb_add(sb, 9, 1)
        n = send
        if fcb_len == n:  # move_into: every slice through add
            for ln, inl in fcb:
                sb_add(sb, ln, inl)
            fcb = []
        else:
            while fcb:
                ln, inl = fcb[0]
                if n >= ln:
                    sb_add(sb, ln, inl)
                    fcb.pop(0)
                    n -= ln
                    if n == 0:
                        break
                else:  # split: the head goes in un-merged (add_indexed), the tail stays
                    sb.append([n, inl])
                    fcb[0][0] = ln - n
                    break
        fcb_len -= send
        off += send
        left -= send


class SendModel:
    def __init__(self, initial_window=65535, conn_window=65535, peer_max_frame=16384):
        self.iws, self.conn, self.pmf = initial_window, conn_window, peer_max_frame
        self.delta = {}    # the table: stream -> credit received - bytes sent
        self.carry = None  # the control frame the previous call's end cut
        self.lost = False
        self.stats = dict(intakes=0, window_updates=0, settings=0, violations=0, frame_calls=0, bytes_sent=0)

    def window(self, sid):
        return self.conn if sid == 0 else self.iws + self.delta.get(sid, 0)

    def _flags(self):
        return LOST if self.lost else 0

    # ---- intake ------------------------------------------------------------------------------------------------------
    def lost_call(self):
        """a call whose event list overflowed: the flag, the carry goes (its frame's end was not seen)"""
        self.lost, self.carry = True, None
        self.stats["intakes"] += 1
        return (0, 0, 0, 0, LOST, 0, len(self.delta), 2)

    def skipped_call(self):
        """a standalone deframing was never taken in: the flag; the next intake starts without a carry"""
        self.lost, self.carry = True, None

    def intake(self, events, slices, err, live):
        """events: the oracle's, tagged with the slice index; slices: the bytes fed; live: the map behind the call"""
        self.stats["intakes"] += 1
        if err:
            return (0, 0, 0, 0, self._flags(), 0, len(self.delta), 0)
        viol, offenders, wus, commits = 0, [], [], []
        cur, self.carry = self.carry, None
        if cur is not None:
            cur["idx"] = 0  # (the carried frame stands in front of the call's events)
        for i, (k, a, b, c, d, sl) in enumerate(events):
            if k == EV_FRAME:
                if a == 0xff:  # (a stream error reported inside a DATA frame's payload)
                    continue
                cur = None
                if (b >> 8) == 0 and (a == 8 or (a == 4 and not (b & 1))):
                    cur = dict(type=a, stream=c, idx=i + 1, bytes=bytearray(), iws=None, mfs=None)
            elif k == EV_PAYLOAD and cur is not None:
                for byte in slices[sl][a:a + b]:
                    cur["bytes"].append(byte)
                    if cur["type"] == 4 and len(cur["bytes"]) == 6:
                        ident, val = struct.unpack(">HI", bytes(cur["bytes"]))
                        cur["bytes"] = bytearray()
                        if ident == 4 and val > MAXW or ident == 5 and not 16384 <= val <= 16777215:
                            viol |= BAD_SETTINGS
                            self.stats["violations"] += 1
                            offenders.append((cur["idx"], 0))
                        elif ident == 4:
                            cur["iws"] = val
                        elif ident == 5:
                            cur["mfs"] = val
                if c:  # is_last
                    if cur["type"] == 8:
                        inc = int.from_bytes(cur["bytes"], "big")
                        if inc == 0 or inc >> 31:
                            viol |= BAD_INCREMENT
                            self.stats["violations"] += 1
                            offenders.append((cur["idx"], cur["stream"]))
                        else:
                            wus.append((cur["idx"], cur["stream"], inc))
                    else:
                        commits.append(cur)
                    cur = None
            else:
                cur = None
        self.carry = cur
        # judged at the end of the call: the map as it is then
        self.delta = {s: v for s, v in self.delta.items() if s in live}
        for f in commits:
            if f["iws"] is not None:
                self.iws = f["iws"]
            if f["mfs"] is not None:
                self.pmf = f["mfs"]
        applied, credit, first = 0, {}, {}
        for idx, s, inc in wus:
            if s == 0 or s in live:
                applied += 1
                credit[s] = credit.get(s, 0) + inc
                first.setdefault(s, idx)
        added_conn = added_streams = 0
        for s, inc in credit.items():
            old = self.conn if s == 0 else self.iws + self.delta.get(s, 0)
            new = old + inc
            if new > MAXW:
                new = max(old, MAXW)
                viol |= WINDOW_OVERFLOW
                self.stats["violations"] += 1
                offenders.append((first[s], s))
            if s == 0:
                added_conn, self.conn = new - old, new
            else:
                added_streams += new - old
                self.delta[s] = new - self.iws
        self.stats["window_updates"] += applied
        self.stats["settings"] += len(commits)
        return (applied, added_conn, added_streams, len(commits), viol | self._flags(),
                min(offenders)[1] if offenders else 0, len(self.delta), 0)

    # ---- framing -----------------------------------------------------------------------------------------------------
    def frame(self, msgs, progress, max_frame, cap, hdr_cap, live):
        """msgs: [(body, stream, flags)]; progress: flow-controlled bytes already sent per message
        -> (slice lengths, wire, result tuple, progress after the call)"""
        self.stats["frame_calls"] += 1
        mf = min(max_frame, self.pmf)
        rem = [5 + len(b) - p for (b, _, _), p in zip(msgs, progress)]
        streams = [s for _, s, _ in msgs]
        for s in streams:
            if s in live:
                self.delta.setdefault(s, 0)  # (a stream the call names has an entry from then on)
        windows = {s: (self.window(s) if s in live else None) for s in streams}
        a, g = grant_prefix(rem, streams, windows, self.conn)
        if g != grant_sequential(rem, streams, windows, self.conn):
            raise AssertionError("the two forms of the grant differ: %r %r %r %d" % (rem, streams, windows, self.conn))
        stall = 0
        for i, s in enumerate(streams):
            if windows[s] is None:
                stall |= STALL_UNKNOWN
            else:
                stall |= (STALL_STREAM if a[i] < rem[i] else 0) | (STALL_CONN if g[i] < a[i] else 0)
        sb, wire = [], bytearray()
        for (body, s, fl), p, gi in zip(msgs, progress, g):
            frame_piece(sb, wire, body, s, fl, mf, p, gi)
        lens = [n for n, _ in sb]
        hdr = 32 * sum(1 for _, inl in sb if inl)
        if len(lens) > cap or hdr > hdr_cap:
            return [], b"", (0, len(msgs), len(lens), hdr, len(wire), 0, stall, 1), list(progress)
        done = sum(1 for r, x in zip(rem, g) if x == r)
        for s, x in zip(streams, g):
            if x:
                self.delta[s] -= x
        self.conn -= sum(g)
        self.stats["bytes_sent"] += sum(g)
        return (lens, bytes(wire), (done, len(msgs) - done, len(lens), hdr, len(wire), sum(g), stall, 0),
                [p + x for p, x in zip(progress, g)])


# ---- where a call's grant lies: what the witnesses of the send-plan sweep read (tests/h2_send_plan_sweep_lib.py) -----------
TILE, BLOCK = 64, 512  # a wave's tile of the plan, the plan's workgroup (H2SW_PLAN_THREADS)


def plan_facts(model, msgs, progress, max_frame, live):
    """what model.frame would decide, without moving anything: per message the remaining bytes, the stream-allowed bytes
    a and the grant g, and the granted pieces [(message index, p, g)] in table order"""
    rem = [5 + len(b) - p for (b, _, _), p in zip(msgs, progress)]
    streams = [s for _, s, _ in msgs]
    windows = {s: (model.window(s) if s in live else None) for s in streams}
    a, g = grant_prefix(rem, streams, windows, model.conn)
    return dict(n=len(msgs), msgs=msgs, p=list(progress), rem=rem, streams=streams, windows=windows, conn=model.conn,
                mf=min(max_frame, model.pmf), a=a, g=g, pieces=[(i, progress[i], x) for i, x in enumerate(g) if x])


def known(f, i):
    return f["windows"][f["streams"][i]] is not None


def tile_lists(f):
    """per tile of 64 messages the streams the map holds, in the order of their last message in the tile: the order of
    the plan's per-tile lists"""
    out = []
    for t0 in range(0, f["n"], TILE):
        last = {}
        for i in range(t0, min(t0 + TILE, f["n"])):
            if known(f, i):
                last[f["streams"][i]] = i
        out.append(sorted(last, key=last.get))
    return out


def stream_end(f, s):
    """-> (i, cut): the window of stream s ends in message i at byte cut of [header | body] (cut == 5 + len: exactly at
    its end, so the stream's next message gets nothing); None where the call's messages do not reach the window's end"""
    left = f["windows"][s]
    for i in range(f["n"]):
        if f["streams"][i] == s:
            if left <= f["rem"][i]:
                return i, f["p"][i] + max(left, 0)
            left -= f["rem"][i]
    return None


def conn_end(f):
    """the same for the connection's window over the stream-allowed bytes"""
    left = f["conn"]
    for i in range(f["n"]):
        if f["a"][i] and left <= f["a"][i]:
            return i, f["p"][i] + max(left, 0)
        left -= f["a"][i]
    return None


def tail_inlined(piece):
    return piece[1] + piece[2] <= 5


def run_before(f, k):
    """how many header-only pieces stand directly in front of piece k"""
    j = k
    while j > 0 and tail_inlined(f["pieces"][j - 1]):
        j -= 1
    return k - j


def back_fill(f, k):
    """the bytes in the outbuf's back slice when piece k begins, 0 where that slice is no inlined one: the run in front
    of the piece through sb_add"""
    sb = []
    for i, p, g in f["pieces"][k - run_before(f, k):k]:
        body, s, fl = f["msgs"][i]
        frame_piece(sb, bytearray(), body, s, fl, f["mf"], p, g)
    return sb[-1][0] if sb and sb[-1][1] else 0


def frames_of(f, k):
    """DATA frames of piece k"""
    return -(-f["pieces"][k][2] // f["mf"])
