"""A sequential model of the receive window ledger (grdma_h2_fc, csrc/grdma_h2_fc.h): the rules of include/grdma_amd.h
applied to the ORACLE's event list (oracle/pyorc.H2Parser.feed), struct.pack for the frames and the 23-byte cut for the
slices.  "Delivered to the stream's data parser" is what the deframer does (parsing.cc init_data_frame_parser): status 0
on a stream that is in the map and open for reads -- the model keeps that set itself, from the streams the test opened
and the oracle's STREAM_OPEN / STREAM_CLOSED events.  Nothing of the library's own events or output goes into it."""
import struct

from oracle.pyorc import EV_FRAME, EV_STREAM_CLOSED, EV_STREAM_OPEN

MAX_INC = (1 << 31) - 1
CONN, STREAM, LOST = 1, 2, 4


class Model:
    def __init__(self, stream_window, conn_window, conn_threshold, max_updates, streams=()):
        self.sw, self.cw, self.thr, self.maxu = stream_window, conn_window, conn_threshold, max_updates
        self.live = set(streams)
        self.announced = conn_window
        self.lost = False
        self.stats = dict(calls=0, conn_bytes=0, stream_bytes=0, frames=0, conn_overflows=0, stream_overflows=0)

    def lost_call(self):
        self.lost = True
        return [], (0, 0, 0, 0, 0, LOST, 0, 2), b""

    def call(self, events, err, slices_cap, hdr_cap):
        """-> (slice lengths, result tuple, wire)"""
        D, S, closed = 0, {}, set()
        for e in events:
            k, a, b, c, d = e[:5]
            if k == EV_FRAME and a == 0:
                D += d
                if (b >> 8) == 0 and c in self.live:
                    S[c] = S.get(c, 0) + d  # (insertion order: the order of the first counted frame)
            elif k == EV_STREAM_OPEN:
                self.live.add(c)
            elif k == EV_STREAM_CLOSED:
                self.live.discard(c)
                closed.add(c)
        viol = CONN if D > 0 and D > self.announced else 0
        self.announced -= D
        violators = [s for s, n in S.items() if n > self.sw]
        if violators:
            viol |= STREAM
        frames = []
        pending = self.cw - self.announced
        if not err and pending > 0 and pending >= self.thr:
            inc = min(pending, MAX_INC)
            frames.append((0, inc))
            self.announced += inc
        if not err:
            frames += [(s, min(n, MAX_INC)) for s, n in S.items() if n > 0 and s not in closed]
        credited = sum(inc for s, inc in frames if s)
        wire = b"".join(struct.pack(">BHBBII", 0, 4, 8, 0, s, inc) for s, inc in frames)
        lens = [min(23, len(wire) - o) for o in range(0, len(wire), 23)]
        over = len(frames) > self.maxu or len(lens) > slices_cap or 32 * len(lens) > hdr_cap
        st = self.stats
        st["calls"] += 1
        st["conn_bytes"] += D
        st["conn_overflows"] += 1 if viol & CONN else 0
        st["stream_overflows"] += len(violators)
        if not over:
            st["stream_bytes"] += credited
            st["frames"] += len(frames)
        res = (len(frames), len(lens), len(wire), D, credited, viol | (LOST if self.lost else 0),
               violators[0] if violators else 0, 1 if over else 0)
        self.frames = frames
        return lens, res, wire
