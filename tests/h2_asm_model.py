"""A sequential model of the message assembler (grdma_h2_asm, csrc/grdma_h2_asm.h): descriptors with their exact offsets,
seqs and statuses, and the bytes of every message, from the deframer's events call by call.  The device plans the same
thing with prefix sums; this walks the events one at a time."""
from oracle.pyorc import EV_MSG_BEGIN, EV_MSG_BYTES, EV_MSG_END, EV_STREAM_CLOSED

OK, TOO_LARGE, NO_SPACE, TRUNCATED = 0, 1, 2, 3
GRANULE = 256


class AsmModel:
    def __init__(self, arena_bytes, max_message_bytes=4 << 20, max_pending=4096):
        self.A, self.max_msg, self.max_pending = arena_bytes, max_message_bytes, max_pending
        self.vh = self.vt = 0
        self.recs = {}            # record number -> [vstart, vend, rank, freed]
        self.rec_head = self.rec_tail = 0
        self.seq = self.reported = self.released = 0
        self.carried = {}         # stream -> open message (dict)

    def release(self, n=None):
        """n=None: everything reported (what a pipe step does first)"""
        self.released = self.reported if n is None else min(self.reported, self.released + n)
        while self.rec_tail < self.rec_head:
            r = self.recs[self.rec_tail]
            if not (r[3] or (r[2] is not None and r[2] < self.released)):
                break
            del self.recs[self.rec_tail]
            self.rec_tail += 1
        self.vt = self.recs[self.rec_tail][0] if self.rec_tail < self.rec_head else self.vh

    def bytes_in_use(self):
        return self.vh - self.vt

    def failed_call(self):
        """a call that failed on the distinct-stream limit: nothing is assembled -- no descriptor, no byte, the ring, the
        records and seq as they were.  The deframer consumed the call's bytes all the same, so what the streams carried
        into the call can never complete: those messages are dropped, their records freed, and never reported."""
        for m in self.carried.values():
            if m["rec"] is not None:
                self.recs[m["rec"]][3] = True
        self.carried = {}

    def call(self, events, slices, h2_error=0):
        """events: (kind, a, b, c, d, slice) with MSG_BYTES offsets inside slices[slice]; -> [(desc tuple, bytes)]
        desc = (offset, length, seq, stream_id, status, flags); bytes = the payload of a complete OK message, else None"""
        A = self.A
        cur = self.vh
        live = self.rec_head - self.rec_tail
        k = 0
        failed = False
        opened = dict(self.carried)
        out = []

        def report(m, status, at_error=False):
            d = (m["offset"] if status == OK else 0, m["length"], m["seq"], m["stream"], status, m["flags"])
            if m["rec"] is not None:
                rec = self.recs[m["rec"]]
                rec[2] = self.reported
                # a truncated message gives its space back at once; a connection error frees every partial record
                rec[3] = rec[3] or status == TRUNCATED or at_error
            self.reported += 1
            out.append((d, bytes(m["data"]) if status == OK else None))

        for e in events:
            kind, a, b, c = e[0], e[1], e[2], e[3]
            if kind == EV_MSG_BEGIN:
                too_large = bool(self.max_msg) and b > self.max_msg
                s = 0 if too_large else (b + GRANULE - 1) // GRANULE * GRANULE
                m = dict(offset=0, length=b, seq=self.seq + k, stream=c, flags=a & 1, rec=None, data=bytearray())
                start = cur
                if s and cur % A + s > A:
                    start = cur + (A - cur % A)
                if failed or k >= self.max_pending - live or (s and start + s - self.vt > A):
                    failed = True
                    m["status"] = NO_SPACE
                else:
                    cur = start + s
                    m["status"] = TOO_LARGE if too_large else OK
                    if s:
                        m["offset"] = start % A
                    m["rec"] = self.rec_head
                    self.recs[self.rec_head] = [start, start + s, None, False]
                    self.rec_head += 1
                k += 1
                opened[c] = m
            elif kind == EV_MSG_BYTES:
                m = opened.get(c)
                if m is not None and m["status"] == OK:
                    sl = slices[e[5]]
                    m["data"] += sl[a:a + b]
            elif kind == EV_MSG_END:
                m = opened.pop(c, None)
                if m is not None:
                    report(m, m["status"])
            elif kind == EV_STREAM_CLOSED:
                m = opened.pop(c, None)
                if m is not None:
                    report(m, TRUNCATED if m["status"] == OK else m["status"])
        if h2_error:
            for m in sorted(opened.values(), key=lambda m: m["seq"]):
                report(m, TRUNCATED if m["status"] == OK else m["status"], at_error=True)
            opened = {}
        self.seq += k
        self.vh = cur
        self.carried = opened
        return out


def oracle_calls(calls, prefix=False, streams=(), max_frame=16384):
    """calls: a list of calls, each a list of slice bytes -> [(h2 error, events with slice indices in the call)];
    an entry ("open", ids) between two calls opens those streams there (a client starting calls) and yields nothing"""
    from oracle import pyorc
    p = pyorc.H2Parser(expect_client_prefix=prefix, max_frame_size=max_frame)
    for sid in streams:
        assert p.open_stream(sid) == 0
    out, err = [], 0
    for slices in calls:
        if isinstance(slices, tuple) and slices[0] == "open":
            for sid in slices[1]:
                assert p.open_stream(sid) == 0
            continue
        ev_call = []
        for i, s in enumerate(slices):
            if err:
                break
            rc, ev = p.feed(s)
            ev_call += [(k, a, b, c, d, i) for k, a, b, c, d in ev]
            err = err or rc
        out.append((err, ev_call))
    return out
