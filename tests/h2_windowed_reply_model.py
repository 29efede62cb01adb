"""A sequential model of replies under the peer's windows (grdma_h2_reply_frame_windowed, csrc/grdma_h2_wr.h): the rules
of include/grdma_amd.h ("Replies under the peer's windows") with the queue as a Python list.  It is driven by what the
assembler's model reported (tests/h2_asm_model.py: AsmModel.call), the routes, the stream map of the outgoing
transport's ORACLE parser (live_of) and SendModel.frame (tests/h2_send_model.py) for the grant and the wire.  Nothing of
the library's output goes into it; tests/test_h2_windowed_reply_model.py pins it before a device test trusts it."""
from tests.h2_asm_model import OK

LOST = 1
WORDS = ("finished", "pending", "slices", "hdr_bytes", "wire_bytes", "granted", "stall", "overflow", "taken_new",
         "dropped_status", "unrouted", "dropped_closed", "releasable", "flags")


class Entry:
    __slots__ = ("body", "stream", "flags", "progress", "rank")

    def __init__(self, body, stream, flags, rank):
        self.body, self.stream, self.flags, self.progress, self.rank = body, stream, flags, 0, rank


class WindowedReplyModel:
    """asm: the source's AsmModel (reported / released are read from it); send: the SendModel of the outgoing
    transport; routes: None (echo) or {from_stream: to_stream}"""

    def __init__(self, asm, send, max_frame=16384, routes=None, max_pending=4096, max_messages=4096):
        self.asm, self.send = asm, send
        self.max_frame, self.routes, self.max_pending, self.max_messages = max_frame, routes, max_pending, max_messages
        self.queue = []        # unfinished entries in order
        self.calls = self.taken = 0
        self.new = None        # the source's last call: (what it reported, rank of its first descriptor, skipped)
        self.lost = False

    # ---- the source ----------------------------------------------------------------------------------------------
    def source_call(self, reported, skipped=False):
        """one standalone call of the source assembler, AFTER AsmModel.call: reported = its [(descriptor, body)];
        skipped: the assembler skipped the call (the event list overflowed), nothing was reported"""
        self.calls += 1
        self.new = (list(reported), self.asm.reported - len(reported), skipped)

    def pending(self):
        return [(e.stream, len(e.body), e.progress) for e in self.queue]

    # ---- a call ----------------------------------------------------------------------------------------------------
    def _releasable(self, stays):
        lim = self.asm.reported
        if stays and not self.new[2]:
            lim = self.new[1]  # (a source call that is new and was not taken is not covered)
        if self.queue:
            lim = min(lim, min(e.rank for e in self.queue))
        return max(0, lim - self.asm.released)

    def frame(self, live, cap, hdr_cap, pending_only=False):
        """live: the streams the outgoing transport's map holds -> (slice lengths, wire, the result words but the time
        and the spare one as a tuple in the order of WORDS)"""
        is_new = self.calls > self.taken
        take = is_new and not pending_only
        if self.calls > self.taken + 1:
            self.lost = True
            self.taken = self.calls - 1
        flags = LOST if self.lost else 0
        closed = status = unrouted = 0
        table = []
        for e in self.queue:
            if e.stream in live:
                table.append(e)
            else:
                closed += 1  # (even one that is partly sent)
        n_old = len(table)
        bad = False
        if take:
            reported, rank_base, skipped = self.new
            bad = skipped or len(reported) > self.max_messages
            for i, (d, body) in enumerate([] if bad else reported):
                if d[4] != OK:
                    status += 1
                    continue
                to = d[3] if self.routes is None else self.routes.get(d[3], 0)
                if to == 0:
                    unrouted += 1
                elif to not in live:
                    closed += 1
                else:
                    table.append(Entry(body, to, d[5] & 1, rank_base + i))
        over = 1 if bad else (2 if len(table) > self.max_pending else 0)
        if over:  # (the plan runs over an empty table: it frames nothing and counts a call)
            self.send.frame([], [], self.max_frame, cap, hdr_cap, live)
            count = len(table) if over == 2 else len(self.queue)
            return [], b"", (0, count, 0, 0, 0, 0, 0, over, 0, 0, 0, 0, self._releasable(is_new), flags)
        lens, wire, r, prog = self.send.frame([(e.body, e.stream, e.flags) for e in table], [e.progress for e in table],
                                              self.max_frame, cap, hdr_cap, live)
        if r[7]:  # a cap: nothing is written, the queue stands, the source call is not taken
            return [], b"", (0, len(self.queue), r[2], r[3], r[4], 0, r[6], 1, 0, 0, 0, 0, self._releasable(is_new), flags)
        for e, p in zip(table, prog):
            e.progress = p
        self.queue = [e for e in table if e.progress < 5 + len(e.body)]
        if take:
            self.taken = self.calls
        return lens, wire, (len(table) - len(self.queue), len(self.queue), r[2], r[3], r[4], r[5], r[6], 0,
                            len(table) - n_old, status, unrouted, closed, self._releasable(is_new and not take), flags)
