"""Device-side HTTP/2 DATA framing / deframing (grdma_h2_*), thin ctypes wrappers."""
import ctypes as C

from ._abi import (H2CtlItem, H2DeframeItem, H2Event, H2FcItem, H2HpackItem, H2HpencItem, H2LinkSpec,  # noqa: F401
                   H2MessagesItem, H2Msg, H2ReplyItem, H2ReplyLinkSpec, H2Route, H2RxMsg, H2SwFrameItem, H2WrItem, ReadSlice,
                   Slice)
from ._lib import GrdmaError, check, load

u64 = C.c_uint64
_bind = load  # (h2dev._bind() is load(): the library with every prototype of _abi.SIGNATURES set; it binds nothing itself)

MSG_OK, MSG_TOO_LARGE, MSG_NO_SPACE, MSG_TRUNCATED = 0, 1, 2, 3
SYNC_KEYS = ("framed", "frame_overflow", "events", "deframe_overflow", "parsed", "h2_error", "frame_us", "deframe_us",
             "bulk_steps", "bulk_frames", "t_wait", "t_bulk", "t_total", "t_serial")


class Msg(tuple):
    """One received gRPC message: (offset, length, seq, stream_id, status, flags)."""
    __slots__ = ()
    _names = ("offset", "length", "seq", "stream_id", "status", "flags")

    def __new__(cls, offset, length, seq, stream_id, status, flags):
        return tuple.__new__(cls, (offset, length, seq, stream_id, status, flags))

    def __getattr__(self, k):
        try:
            return self[Msg._names.index(k)]
        except ValueError:
            raise AttributeError(k)

    def __repr__(self):
        return "Msg(%s)" % ", ".join("%s=%d" % (k, v) for k, v in zip(Msg._names, self))


def _msgs(arr, n):
    return [Msg(int(m.offset), int(m.length), int(m.seq), int(m.stream_id), int(m.status), int(m.flags)) for m in arr[:n]]


def _msg_array(msgs):
    """[(payload device ptr, len, stream_id, flags), ...] as an H2Msg array (never of length 0)"""
    arr = (H2Msg * max(1, len(msgs)))()
    for i, (p, n, sid, fl) in enumerate(msgs):
        arr[i].payload, arr[i].len, arr[i].stream_id, arr[i].flags = p, n, sid, fl
    return arr


def _slice_array(slices):
    """[(offset, len), ...] as a ReadSlice array (never of length 0)"""
    arr = (ReadSlice * max(1, len(slices)))()
    for i, (o, l) in enumerate(slices):
        arr[i].off, arr[i].len = o, l
    return arr


def _events(arr, m):
    return [(e.kind, e.a, e.b, e.c, e.d, e.slice) for e in arr[:m]]


def _read_slice_table(lib, slices_ptr, n):
    """the first n rows of a slice table in device memory -> [(ptr, len), ...]"""
    raw = C.create_string_buffer(max(1, 16 * n))
    if n:
        check(lib.grdma_copy_to_host(raw, slices_ptr, 16 * n))
    return [(int.from_bytes(raw.raw[16 * i:16 * i + 8], "little"), int.from_bytes(raw.raw[16 * i + 8:16 * i + 16], "little"))
            for i in range(n)]


def _read_wire(lib, slices):
    """the bytes the slices [(device ptr, len), ...] point to, in their order"""
    wire = b""
    for ptr, ln in slices:
        buf = C.create_string_buffer(max(1, ln))
        check(lib.grdma_copy_to_host(buf, ptr, ln))
        wire += buf.raw[:ln]
    return wire


def _results(out, objs, words=8):
    """the result words `out` of a call cut into one tuple per object, each also left in its object's .last_result"""
    res = [tuple(int(x) for x in out[words * i:words * i + words]) for i in range(len(objs))]
    for o, r in zip(objs, res):
        o.last_result = r
    return res


def _items(cls, items):
    """the items [(object, value, ...), ...] of a batch call as an array of the ABI struct `cls` (never of length 0): the
    first field takes the object's handle (None for no object), the fields that follow it the values, in the struct's
    order; an item that is None stays zero"""
    first, *rest = [n for n, _ in cls._fields_]
    arr = (cls * max(1, len(items)))()
    for a, item in zip(arr, items):
        if item is not None:
            setattr(a, first, item[0].h if item[0] is not None else None)
            for name, v in zip(rest, item[1:]):
                setattr(a, name, v)
    return arr


def _batch(call, arr, items):
    """a batch call that writes eight result words per item -> (what it returned, [result tuple per item]); the tuples
    also land in the .last_result of each item's object"""
    out = (u64 * (8 * max(1, len(items))))()
    rc = check(call(arr, len(items), out))
    return rc, _results(out, [item[0] for item in items])


class _Handle:
    """One grdma_h2_<KIND>_* object of the library (.lib, .h) and what all kinds do alike."""

    KIND = WHAT = None
    last_result = None

    def _fn(self, name):
        return getattr(self.lib, "grdma_h2_%s_%s" % (self.KIND, name))

    def _create(self, *args, error=None):
        """grdma_h2_<KIND>_create(*args) -> .h; a refusal raises with `error` or, without one, in the library's words"""
        self.lib = load()
        self.h = self._fn("create")(*args)
        if not self.h:
            raise GrdmaError(error or "%s: %s" % (self.WHAT, (self.lib.grdma_last_error() or b"creation failed").decode()))

    def _call(self, name, *args):
        """grdma_h2_<KIND>_<name>(handle, *args, eight result words) -> what it returned; the words are in .last_result
        before a failure raises"""
        out = (u64 * 8)()
        n = self._fn(name)(self.h, *args, out)
        _results(out, [self])
        return check(n)

    def _words(self, name, keys):
        """the words grdma_h2_<KIND>_<name> reports (at most eight) as a dict"""
        out = (u64 * 8)()
        check(self._fn(name)(self.h, out))
        return dict(zip(keys, [int(x) for x in out]))

    def _stats(self):
        r = self._words("stats", self.STATS)
        r["kernel_us"] /= 1e3  # (the ABI word is nanoseconds)
        return r

    def close(self):
        if self.h:
            self._fn("destroy")(self.h)
            self.h = None


def frame_messages(msgs, max_frame, slices_dev_ptr, slices_cap, hdr_dev_ptr, hdr_cap):
    """msgs: list of (payload device ptr, len, stream_id, flags). -> (nslices, wire_bytes)."""
    lib = load()
    wire = u64(0)
    n = check(lib.grdma_h2_frame_messages(_msg_array(msgs), len(msgs), max_frame, slices_dev_ptr, slices_cap,
                                          hdr_dev_ptr, hdr_cap, C.byref(wire)))
    return n, wire.value


H2_SERVER, H2_FIRST_FRAME, H2_BOUNDARY_STEP, H2_NO_BOUNDARY_STEP, H2_BULK_PAIRS, H2_TICKS, H2_NO_BULK_PAIRS = 1, 2, 4, 8, 16, 32, 64
H2_NO_CHUNKS = 128


class Parser(_Handle):
    """Deframe state + stream map of one transport in device memory (grdma_h2_parser).
    expect_client_prefix=True: a fresh server connection (streams accepted from HEADERS);
    False: a client / mid-connection parser whose streams the caller opens."""

    KIND = "parser"  # grdma_h2_parser_destroy

    def __init__(self, expect_client_prefix=False, max_frame_size=16384, flags=None,
                 max_concurrent_streams=0xFFFFFFFF, table_slots=0, boundary_step=None, bulk_pairs=None, ticks=False, chunks=None):
        self.lib = load()
        if flags is None:
            flags = (H2_SERVER | H2_FIRST_FRAME) if expect_client_prefix else 0
        if boundary_step is not None:  # None: GRDMA_H2_BOUNDARY_STEP in the environment decides
            flags |= H2_BOUNDARY_STEP if boundary_step else H2_NO_BOUNDARY_STEP
        if bulk_pairs is not None:  # None: the library default (64 frames per bulk step unless GRDMA_H2_BULK_PAIRS=0)
            flags |= H2_BULK_PAIRS if bulk_pairs else H2_NO_BULK_PAIRS
        if ticks:
            flags |= H2_TICKS
        if chunks is not None and not chunks:  # None / True: the library default (GRDMA_H2_CHUNKS, lists of >= 2048 slices)
            flags |= H2_NO_CHUNKS
        self.h = self.lib.grdma_h2_parser_create_ex(flags, max_frame_size, max_concurrent_streams, table_slots)
        if not self.h:
            raise GrdmaError("h2 parser allocation failed")

    def _ids(self, ids):
        ids = list(ids)
        return (C.c_uint32 * max(1, len(ids)))(*ids), len(ids)

    def open_streams(self, ids):
        arr, n = self._ids(ids)
        return check(self.lib.grdma_h2_parser_open_streams(self.h, arr, n))

    def close_writes(self, ids):
        arr, n = self._ids(ids)
        return check(self.lib.grdma_h2_parser_close_writes(self.h, arr, n))

    def live_streams(self):
        return check(self.lib.grdma_h2_parser_live_streams(self.h))

    def chunk_stats(self):
        """(calls the chunked deframer planned, calls whose chunks verified and were merged)"""
        out = (u64 * 2)()
        check(self.lib.grdma_h2_parser_chunk_stats(self.h, out))
        return int(out[0]), int(out[1])

    def chunk_phases(self, kmax=256):
        """profiling aid: per chunk (start, cuts found, map copied, parsed, compared, slices) and the merge's stamps, in device-clock ticks relative to the earliest"""
        n = (kmax + 1) * 8
        out = (u64 * n)()
        check(self.lib.grdma_h2_parser_chunk_dbg(self.h, out, n))
        rows = [[int(out[r * 8 + c]) for c in range(8)] for r in range(kmax + 1)]
        return rows

    def deframe(self, arena_dev_ptr, slices, cap=None):
        """slices: list of (offset, len) in the arena. -> (h2 error, events)"""
        n = len(slices)
        arr = _slice_array(slices)
        cap = cap or (sum(l for _, l in slices) * 2 + 64 if n else 64)
        cap = min(cap, 1 << 20)
        ev = (H2Event * cap)()
        err = C.c_int(0)
        m = check(self.lib.grdma_h2_deframe(self.h, arena_dev_ptr, arr, n, ev, cap, C.byref(err)))
        self.last_boundary_steps = int(self.lib.grdma_h2_last_boundary_steps())
        st = (u64 * 8)()
        self.lib.grdma_h2_last_deframe_stats(st)
        self.last_bulk_steps, self.last_bulk_frames = int(st[0]), int(st[1])  # bulk steps taken, frames parsed in them
        return err.value, _events(ev, m)

    def deframe_messages(self, arena_dev_ptr, slices, assembler, want_events=False, ev_cap=None, msgs_cap=None):
        """deframe + assemble: -> (h2 error, [Msg...]) or (h2 error, [Msg...], events) with want_events"""
        n = len(slices)
        arr = _slice_array(slices)
        ev_cap = ev_cap or min(sum(l for _, l in slices) * 2 + 64 if n else 64, 1 << 20)
        msgs_cap = msgs_cap or ev_cap
        ev = (H2Event * ev_cap)() if want_events else None
        out = (H2RxMsg * msgs_cap)()
        err = C.c_int(0)
        m = check(self.lib.grdma_h2_deframe_messages(self.h, assembler.h, arena_dev_ptr, arr, n, ev, ev_cap, out, msgs_cap,
                                                     C.byref(err)))
        msgs = _msgs(out, m)
        if not want_events:
            return err.value, msgs
        return err.value, msgs, [e for e in _events(ev, ev_cap) if e[0]]


def deframe_batch(items, caps=None):
    """The delivered slices of many transports in ONE launch (grdma_h2_deframe_batch).  items: [(Parser, arena device
    ptr, [(offset, len), ...]), ...] with distinct parsers; caps: event capacity per item (default: what
    Parser.deframe takes).  -> [(h2 error, events), ...] per item; every item reports for itself: where the events did
    not fit the item's capacity, `events` is the integer -GRDMA_ERR_CAPACITY (-5) instead of a list."""
    lib = load()
    n = len(items)
    arr = (H2DeframeItem * max(1, n))()
    keep = []
    for i, (parser, arena, slices) in enumerate(items):
        sl = _slice_array(slices)
        cap = (caps[i] if caps is not None else None) or min(sum(l for _, l in slices) * 2 + 64, 1 << 20)
        ev = (H2Event * cap)()
        keep.append((sl, ev))
        arr[i].parser, arr[i].d_arena, arr[i].slices, arr[i].n = parser.h, arena, sl, len(slices)
        arr[i].events_out, arr[i].cap = ev, cap
    check(lib.grdma_h2_deframe_batch(arr, n))
    out = []
    for i in range(n):
        m = int(arr[i].n_events)
        out.append((int(arr[i].h2_error), _events(keep[i][1], m) if m >= 0 else m))
    return out


def deframe_messages_batch(items, want_events=False, ev_caps=None, msgs_caps=None):
    """deframe + assemble for many transports in seven launches (grdma_h2_deframe_messages_batch).  items: [(Parser,
    Assembler, arena device ptr, [(offset, len), ...]), ...] with distinct parsers and assemblers; ev_caps / msgs_caps:
    per item (default: what Parser.deframe_messages takes).  -> per item (h2 error, [Msg...]) or, with want_events,
    (h2 error, [Msg...], events); every item reports for itself: where its events or descriptors did not fit, the
    list is the integer -GRDMA_ERR_CAPACITY (-5) instead."""
    lib = load()
    n = len(items)
    arr = (H2MessagesItem * max(1, n))()
    keep = []
    for i, (parser, asm, arena, slices) in enumerate(items):
        sl = _slice_array(slices)
        cap = (ev_caps[i] if ev_caps is not None else None) or min(sum(l for _, l in slices) * 2 + 64, 1 << 20)
        mcap = (msgs_caps[i] if msgs_caps is not None else None) or cap
        ev = (H2Event * cap)() if want_events else None
        out = (H2RxMsg * mcap)()
        keep.append((sl, ev, out))
        arr[i].parser, arr[i].d_arena, arr[i].slices, arr[i].n = parser.h, arena, sl, len(slices)
        arr[i].events_out, arr[i].cap = ev, cap
        arr[i].assembler, arr[i].msgs_out, arr[i].msgs_cap = (asm.h if asm is not None else None), out, mcap
    check(lib.grdma_h2_deframe_messages_batch(arr, n))
    res = []
    for i in range(n):
        m, k = int(arr[i].n_msgs), int(arr[i].n_events)
        r = (int(arr[i].h2_error), _msgs(keep[i][2], m) if m >= 0 else m)
        if want_events:
            r += (_events(keep[i][1], k) if k >= 0 else k,)
        res.append(r)
    return res


def release_batch(pairs):
    """Assembler.release for many assemblers in one launch (grdma_h2_asm_release_batch): [(Assembler, n), ...]"""
    lib = load()
    n = len(pairs)
    hs = (C.c_void_p * max(1, n))(*[a.h for a, _ in pairs])
    cs = (u64 * max(1, n))(*[c for _, c in pairs])
    check(lib.grdma_h2_asm_release_batch(hs, cs, n))


def reply_frame_batch(items):
    """Reply.frame for many transports in two launches (grdma_h2_reply_frame_batch).  items: [(Reply, slices device ptr,
    slices cap, header arena device ptr, header cap), ...] with distinct replies of distinct, unattached source
    assemblers.  -> per item (slice count, dict of Reply.REPLY_STATS); every item reports for itself: where its caps
    overflowed, the count is the integer -GRDMA_ERR_CAPACITY (-5) and nothing of that item was written.  frame_us is
    the batch's, repeated.  The stats also land in each Reply's .last_stats."""
    arr = _items(H2ReplyItem, items)
    check(load().grdma_h2_reply_frame_batch(arr, len(items)))
    res = []
    for i in range(len(items)):
        st = dict(zip(Reply.REPLY_STATS, [int(x) for x in arr[i].out]))
        items[i][0].last_stats = st
        res.append((int(arr[i].n_slices), st))
    return res


class GroupPipe:
    """frame -> multi-link job -> deframe for several links of ONE job (grdma_h2_group_pipe): one framing kernel and
    one deframing kernel per step however many links.  specs: [(link, msgs, Parser, delivered_slices, events_cap), ...]
    with msgs = [(payload device ptr, len, stream_id, flags), ...]; links and parsers distinct; the job has run once.
    Links that are not listed are carried as before."""

    @classmethod
    def reply(cls, job_back, specs):
        """A group pipe whose framing stage is one Reply per link (grdma_h2_group_pipe_create_reply): a step frames, per
        link, what the last enqueued step of that reply's forward pipe reported, sends it through `job_back` and
        deframes it.  specs: [(link, Reply, back Parser, delivered_slices, events_cap, recorded_wire_bytes), ...].  A
        link whose step has another shape than the job's recorded run keeps its table and reports frame_overflow 2; the
        others go on.  Close it before the forward pipes and before the replies."""
        self = cls.__new__(cls)
        self.lib = load()
        specs = list(specs)
        arr = (H2ReplyLinkSpec * max(1, len(specs)))()
        self._keep = []
        for i, (link, reply, parser, delivered, cap, wire) in enumerate(specs):
            self._keep.append((reply, parser))
            arr[i].link, arr[i].reply = link, (reply.h if reply is not None else None)
            arr[i].parser_back = parser.h if parser is not None else None
            arr[i].delivered_slices, arr[i].events_cap, arr[i].recorded_wire_bytes = delivered, cap, wire
        self.n = len(specs)
        self.events_caps = [sp[4] for sp in specs]
        self.job = job_back
        self.h = self.lib.grdma_h2_group_pipe_create_reply(job_back.h if job_back is not None else None, arr, len(specs))
        if not self.h:
            raise GrdmaError("h2 group reply pipe refused: %s" % self.lib.grdma_last_error().decode())
        self.reply_framers = [sp[1] for sp in specs]
        for r in self.reply_framers:
            r.assembler._reply_pipes = getattr(r.assembler, "_reply_pipes", 0) + 1
        return self

    def __init__(self, job, specs, max_frame=16384):
        self.lib = load()
        specs = list(specs)
        arr = (H2LinkSpec * max(1, len(specs)))()
        self._keep = []
        for i, (link, msgs, parser, delivered, cap) in enumerate(specs):
            m = _msg_array(msgs)
            self._keep.append((m, parser))
            arr[i].link, arr[i].msgs, arr[i].nmsgs, arr[i].parser = link, m, len(msgs), parser.h
            arr[i].delivered_slices, arr[i].events_cap = delivered, cap
        self.n = len(specs)
        self.events_caps = [sp[4] for sp in specs]
        self.job = job  # (kept alive)
        self.h = self.lib.grdma_h2_group_pipe_create(job.h, arr, len(specs), max_frame)
        if not self.h:
            raise GrdmaError("h2 group pipe refused: %s" % self.lib.grdma_last_error().decode())

    def enqueue(self):
        check(self.lib.grdma_h2_group_pipe_enqueue(self.h))

    def sync(self):
        """-> one dict per spec with the keys of Pipe.sync (frame_us / deframe_us are the batch's)"""
        out = (u64 * (14 * self.n))()
        check(self.lib.grdma_h2_group_pipe_sync(self.h, out, 14 * self.n))
        return [dict(zip(SYNC_KEYS, [int(x) for x in out[14 * i:14 * i + 14]])) for i in range(self.n)]

    def events(self, i):
        cap = max(1, self.events_caps[i])
        ev = (H2Event * cap)()
        m = check(self.lib.grdma_h2_group_pipe_events(self.h, i, ev, cap))
        return _events(ev, m)

    def slice_table(self, i, cap=1 << 16):
        arr = (Slice * cap)()
        n = check(self.lib.grdma_h2_group_pipe_slice_table(self.h, i, arr, cap))
        return [(int(arr[k].ptr or 0), int(arr[k].len)) for k in range(n)]

    def hook_counts(self):
        """(kernels in front of, kernels behind) the job's rounds inside its graph"""
        return job_hook_counts(self.job)

    def attach_assemblers(self, asms):
        """one Assembler (of the spec's parser) or None per spec: every later step assembles the messages of those
        links, six more kernels however many links (grdma_h2_group_pipe_attach_assemblers).  Close the pipe before
        the assemblers."""
        asms = list(asms)
        hs = (C.c_void_p * max(1, len(asms)))(*[a.h if a is not None else None for a in asms])
        check(self.lib.grdma_h2_group_pipe_attach_assemblers(self.h, hs, len(asms)))
        self.assemblers = asms  # (kept alive)

    def messages(self, i, cap=None):
        """the messages of spec i in the last synced step"""
        cap = cap or max(1, self.events_caps[i])
        out = (H2RxMsg * cap)()
        m = check(self.lib.grdma_h2_group_pipe_messages(self.h, i, out, cap))
        return _msgs(out, m)

    def attach_flow_control(self, fcs):
        """one FlowControl (of the spec's parser) or None per spec: every later step accounts the events of those links,
        five more kernels however many links (grdma_h2_group_pipe_attach_flow_control).  The pipe refuses a parser that
        has a ledger when it is created: create the pipe, then the FlowControl on the link's parser, then attach.
        Close the pipe before the ledgers."""
        fcs = list(fcs)
        hs = (C.c_void_p * max(1, len(fcs)))(*[f.h if f is not None else None for f in fcs])
        check(self.lib.grdma_h2_group_pipe_attach_flow_control(self.h, hs, len(fcs)))
        self.flow_controls = fcs  # (kept alive)
        for f in fcs:
            if f is not None:
                f._pipe = self

    def window_updates(self, i):
        """the window-update list of spec i in the last step -> ([(ptr, len), ...], result tuple, wire bytes)"""
        fcs = getattr(self, "flow_controls", [])
        fc = fcs[i] if i < len(fcs) else None
        cap = (13 * fc.max_updates + 22) // 23 if fc is not None else 0   # (a spec without ledger: the call refuses)
        arr = (Slice * max(1, cap))()
        out = (u64 * 8)()
        n = self.lib.grdma_h2_group_pipe_window_updates(self.h, i, arr, cap, out)
        res = tuple(int(x) for x in out)
        n = check(n)
        buf = C.create_string_buffer(max(1, res[2]))
        m = check(self.lib.grdma_h2_group_pipe_window_update_bytes(self.h, i, buf, res[2]))
        return [(int(arr[k].ptr or 0), int(arr[k].len)) for k in range(n)], res, buf.raw[:m]

    def close(self):
        """does nothing while a reply pipe reads one of this pipe's assemblers (grdma_h2_group_pipe_destroy does not
        either): close that one first, then call close again"""
        if self.h:
            if any(a is not None and getattr(a, "_reply_pipes", 0) for a in getattr(self, "assemblers", [])):
                return
            self.lib.grdma_h2_group_pipe_destroy(self.h)
            self.h = None
            for f in getattr(self, "flow_controls", []):
                if f is not None:
                    f._pipe = None
            self.flow_controls = []
            for r in getattr(self, "reply_framers", []):
                r.assembler._reply_pipes -= 1
            self.reply_framers = []


def job_hook_counts(job):
    out = (C.c_uint32 * 2)()
    check(load().grdma_job_hook_counts(job.h, out))
    return int(out[0]), int(out[1])


class Assembler(_Handle):
    """Received gRPC messages, contiguous in a ring over `arena` (grdma_h2_asm): a DeviceBuffer-like object (.ptr,
    .nbytes) or a torch uint8 tensor on the device.  max_message_bytes = 0: no limit."""

    KIND = "asm"  # grdma_h2_asm_create, grdma_h2_asm_destroy

    def __init__(self, parser, arena, max_message_bytes=4 << 20, max_pending=4096):
        self.parser = parser  # (kept alive)
        self.arena = arena
        if hasattr(arena, "data_ptr"):
            ptr, size = arena.data_ptr(), arena.numel() * arena.element_size()
        else:
            ptr, size = arena.ptr, arena.nbytes
        self.ptr, self.size = ptr, size
        self._create(parser.h, ptr, size, max_message_bytes, max_pending, error="h2 assembler creation failed")

    def release(self, n):
        check(self.lib.grdma_h2_asm_release(self.h, n))

    def stats(self):
        """dict(reported, ok_bytes, too_large, no_space, truncated, bytes_in_use, plan_us, copy_us)"""
        return self._words("stats", ("reported", "ok_bytes", "too_large", "no_space", "truncated", "bytes_in_use", "plan_us",
                                     "copy_us"))  # grdma_h2_asm_stats

    def last_call(self):
        """(descriptors device ptr, their number, events device ptr, their number) of the last deframe_messages through
        this assembler: what CallTable.step takes with no table copied through the host; valid until the parser's next
        deframing"""
        out = (u64 * 4)()
        check(self.lib.grdma_h2_asm_last_call(self.h, out))
        return tuple(int(x) for x in out)

    def view(self, msg):
        """the bytes of an OK message: a slice of the arena tensor, or bytes read back from the device"""
        if hasattr(self.arena, "data_ptr"):
            return self.arena[msg.offset:msg.offset + msg.length]
        if not msg.length:
            return b""
        dst = C.create_string_buffer(msg.length)
        check(self.lib.grdma_copy_to_host(dst, self.ptr + msg.offset, msg.length))
        return dst.raw[:msg.length]


class Reply(_Handle):
    """Replies framed on the device from the descriptors of `assembler`'s last call (grdma_h2_reply): every OK message
    back on its own stream (routes=None), or the messages of the streams in routes = [(from_stream, to_stream), ...]
    on their to_stream and the others dropped.  Slices point into the assembler's arena: release behind the send."""

    KIND = "reply"  # grdma_h2_reply_create, grdma_h2_reply_destroy
    REPLY_STATS = ("kept", "dropped_status", "unrouted", "slices", "hdr_bytes", "wire_bytes", "overflow", "frame_us")

    def __init__(self, assembler, routes=None, max_frame=16384, max_messages=4096):
        self.assembler = assembler  # (kept alive)
        routes = list(routes or [])
        arr = (H2Route * max(1, len(routes)))()
        for i, (a, b) in enumerate(routes):
            arr[i].from_stream, arr[i].to_stream = a, b
        self._create(assembler.h, arr if routes else None, len(routes), max_frame, max_messages,
                     error="h2 reply creation failed (a duplicate or zero stream id in the routes, more than 4096 of them, "
                           "max_frame or max_messages out of range)")
        self.last_stats = None

    def frame(self, slices_ptr, cap, hdr_ptr, hdr_cap):
        """-> (slice count, dict of REPLY_STATS); raises GrdmaError (capacity) when a cap overflows -- the stats of the
        failed call stay in .last_stats"""
        out = (u64 * 8)()
        n = self.lib.grdma_h2_reply_frame(self.h, slices_ptr, cap, hdr_ptr, hdr_cap, out)
        self.last_stats = dict(zip(Reply.REPLY_STATS, [int(x) for x in out]))
        return check(n), self.last_stats

    # ---- under the peer's windows (grdma_h2_reply_attach_windows / _frame_windowed) -----------------------------------
    WINDOWED = ("finished", "pending", "slices", "hdr_bytes", "wire_bytes", "granted", "stall", "overflow", "taken_new",
                "dropped_status", "unrouted", "dropped_closed", "releasable", "flags", "frame_us", "spare")
    PENDING_ONLY, LOST = 1, 1

    def attach_windows(self, sw, max_pending=4096):
        """binds the reply to the SendWindows of the transport its replies go out on and allocates the queue of what the
        windows cut off; from then on frame_windowed frames, frame is refused"""
        rc = self.lib.grdma_h2_reply_attach_windows(self.h, sw.h if sw is not None else None, max_pending)
        if rc < 0:
            raise GrdmaError("h2 windowed reply: " + (self.lib.grdma_last_error() or b"attach failed").decode())
        self.send_windows = sw  # (kept alive)

    def frame_windowed(self, slices_ptr, cap, hdr_ptr, hdr_cap, pending_only=False):
        """what waited, then (unless pending_only) what the assembler's last call brought, under the windows ->
        ([(ptr, len), ...], dict of WINDOWED); raises GrdmaError on a refusal or an overflow -- the result of the failed
        call stays in .last_windowed, nothing was sent, the queue stands"""
        out = (u64 * 16)()
        n = self.lib.grdma_h2_reply_frame_windowed(self.h, Reply.PENDING_ONLY if pending_only else 0, slices_ptr, cap,
                                                   hdr_ptr, hdr_cap, out)
        self.last_windowed = dict(zip(Reply.WINDOWED, [int(x) for x in out]))
        n = check(n)
        return _read_slice_table(self.lib, slices_ptr, n), self.last_windowed

    def pending(self):
        """the queue as it is: [(outgoing stream, message length, flow-controlled bytes sent), ...] in its order"""
        n = check(self.lib.grdma_h2_reply_pending(self.h, None, 0))
        out = (u64 * max(1, 3 * n))()
        n = check(self.lib.grdma_h2_reply_pending(self.h, out, n))
        return [(int(out[3 * i]), int(out[3 * i + 1]), int(out[3 * i + 2])) for i in range(n)]


def reply_frame_windowed_batch(items):
    """Reply.frame_windowed for many transports in four launches (grdma_h2_reply_frame_windowed_batch).  items: [(Reply,
    slices device ptr, slices cap, header arena device ptr, header cap, pending_only), ...] with distinct replies of
    distinct source assemblers, each attached to its own SendWindows.  -> per item (slice list, or the integer
    -GRDMA_ERR_CAPACITY (-5) where that item overflowed and nothing of it was written; dict of Reply.WINDOWED).  frame_us
    is the batch's, repeated.  The results also land in each Reply's .last_windowed."""
    lib = load()
    # (H2WrItem's fields in their order: reply, flags, pad, the four target fields)
    arr = _items(H2WrItem, [(reply, Reply.PENDING_ONLY if pending_only else 0, 0, *target) for reply, *target, pending_only in items])
    check(lib.grdma_h2_reply_frame_windowed_batch(arr, len(items)))
    res = []
    for i in range(len(items)):
        st = dict(zip(Reply.WINDOWED, [int(x) for x in arr[i].out]))
        items[i][0].last_windowed = st
        k = int(arr[i].n_slices)
        res.append((_read_slice_table(lib, items[i][1], k) if k >= 0 else k, st))
    return res


FC_CONN_OVERFLOW, FC_STREAM_OVERFLOW, FC_LOST = 1, 2, 4


class FlowControl(_Handle):
    """Receive flow control of one transport on the device (grdma_h2_fc): the DATA bytes of a deframing counted
    against stream_window / conn_window, and the WINDOW_UPDATE frames that return them.  One per parser."""

    KIND, WHAT = "fc", "h2 flow control"  # grdma_h2_fc_create, grdma_h2_fc_destroy
    RESULT = ("frames", "slices", "wire_bytes", "conn_bytes", "stream_bytes", "violations", "first_violator", "overflow")
    STATS = ("calls", "conn_bytes", "stream_bytes", "frames", "conn_overflows", "stream_overflows", "announced", "kernel_us")

    def __init__(self, parser, stream_window=65535, conn_window=65535, conn_threshold=0, max_updates=4096):
        self.parser = parser  # (kept alive)
        self.max_updates = max_updates
        self._create(parser.h, stream_window, conn_window, conn_threshold, max_updates)

    def account(self, slices_ptr, cap, hdr_ptr, hdr_cap):
        """accounts the parser's last standalone deframing -> ([(ptr, len), ...], result tuple (RESULT), wire bytes);
        raises GrdmaError on a refusal or a capacity overflow -- the result of the failed call stays in .last_result"""
        sl = _read_slice_table(self.lib, slices_ptr, self._call("account", slices_ptr, cap, hdr_ptr, hdr_cap))  # grdma_h2_fc_account
        return sl, self.last_result, _read_wire(self.lib, sl)

    def stats(self):
        """dict of STATS; `lost`: the sticky flag; announced: the connection window the peer knows (may be negative)"""
        r = self._stats()  # grdma_h2_fc_stats
        r["lost"] = bool(r["stream_overflows"] >> 63)
        r["stream_overflows"] &= (1 << 63) - 1
        r["announced"] = r["announced"] - (1 << 64) if r["announced"] >> 63 else r["announced"]
        return r

    def close(self):
        """does nothing while a pipe has the ledger attached (close the pipe first)"""
        if self.h and not getattr(self, "_pipe", None):
            self.lib.grdma_h2_fc_destroy(self.h)
            self.h = None


class SendWindows(_Handle):
    """Send flow control of one transport on the device (grdma_h2_sw): the peer's windows, fed from the parser's
    deframings (intake), and grdma_h2_frame_messages under them (frame).  One per parser."""

    KIND, WHAT = "sw", "h2 send windows"  # grdma_h2_sw_create, grdma_h2_sw_destroy
    INTAKE = ("window_updates", "conn_credit", "stream_credit", "settings", "violations", "first_offender", "live_entries",
              "overflow")
    FRAME = ("completed", "held", "slices", "hdr_bytes", "wire_bytes", "granted", "stall", "overflow")
    STATS = ("intakes", "window_updates", "settings", "violations", "frame_calls", "bytes_sent", "peer_settings", "kernel_us")
    BAD_INCREMENT, WINDOW_OVERFLOW, BAD_SETTINGS, LOST = 1, 2, 4, 8

    def __init__(self, parser, initial_window=65535, conn_window=65535, peer_max_frame=16384):
        self.parser = parser  # (kept alive)
        self._create(parser.h, initial_window, conn_window, peer_max_frame)

    def intake(self):
        """takes in the parser's last standalone deframing -> result tuple (INTAKE); raises GrdmaError on a refusal or a
        lost call -- the result of the failed call stays in .last_result"""
        self._call("intake")  # grdma_h2_sw_intake
        return self.last_result

    def frame(self, msgs, progress, max_frame, slices_ptr, cap, hdr_ptr, hdr_cap):
        """msgs: [(payload device ptr, len, stream_id, flags), ...]; progress: flow-controlled bytes already sent per
        message -> ([(ptr, len), ...], result tuple (FRAME), progress after the call); raises GrdmaError on a refusal or
        a capacity overflow -- the result of the failed call stays in .last_result, nothing was sent"""
        n = len(msgs)
        prog = (u64 * max(1, n))(*progress)
        k = self._call("frame", _msg_array(msgs), prog, n, max_frame, slices_ptr, cap, hdr_ptr, hdr_cap)  # grdma_h2_sw_frame
        return _read_slice_table(self.lib, slices_ptr, k), self.last_result, [int(x) for x in prog[:n]]

    def windows(self, ids):
        """the windows as they are: id 0 is the connection's, another id its stream's (may be negative)"""
        ids = list(ids)
        arr = (C.c_uint32 * max(1, len(ids)))(*ids)
        out = (C.c_int64 * max(1, len(ids)))()
        check(self.lib.grdma_h2_sw_windows(self.h, arr, len(ids), out))
        return [int(x) for x in out[:len(ids)]]

    def stats(self):
        """dict of STATS plus `lost` (the sticky flag), `initial_window` and `max_frame` (the peer's settings)"""
        r = self._stats()  # grdma_h2_sw_stats
        r["lost"] = bool(r["violations"] >> 63)
        r["violations"] &= (1 << 63) - 1
        r["initial_window"], r["max_frame"] = r["peer_settings"] & 0xffffffff, r.pop("peer_settings") >> 32
        return r


class ControlReplies(_Handle):
    """The control replies of one transport on the device (grdma_h2_ctl): SETTINGS ACK, PING ACK and RST_STREAM written
    from the parser's deframings, and the record of what the peer said.  One per parser; independent of FlowControl and
    SendWindows, which may consume the same deframing."""

    KIND, WHAT = "ctl", "h2 control replies"  # grdma_h2_ctl_create, grdma_h2_ctl_destroy
    RESULT = ("frames", "slices", "wire_bytes", "settings_acks", "ping_acks", "rst_streams", "flags", "overflow")
    PEER = ("settings_acks", "ping_acks", "last_ping_opaque", "goaways", "goaway_last_stream", "goaway_error", "goaway_call")
    STATS = ("calls", "settings_acks", "ping_acks", "rst_streams", "wire_bytes", "reserved", "lost", "kernel_us")
    LOST, GOAWAY = 1, 2

    def __init__(self, parser, max_replies=4096):
        self.parser = parser  # (kept alive)
        self._create(parser.h, max_replies)

    def reply(self, slices_ptr, cap, hdr_ptr, hdr_cap):
        """answers the parser's last standalone deframing -> ([(ptr, len), ...], result tuple (RESULT)); raises
        GrdmaError on a refusal, a lost call or a capacity overflow -- the result of the failed call stays in
        .last_result; after a capacity overflow (overflow word 1) the call may be repeated with larger targets"""
        n = self._call("reply", slices_ptr, cap, hdr_ptr, hdr_cap)  # grdma_h2_ctl_reply
        return _read_slice_table(self.lib, slices_ptr, n), self.last_result

    def peer(self):
        """dict of PEER: what the peer said so far"""
        return self._words("peer", ControlReplies.PEER)  # grdma_h2_ctl_peer

    def stats(self):
        """dict of STATS; `lost`: the sticky flag"""
        r = self._stats()  # grdma_h2_ctl_stats
        r.pop("reserved")
        r["lost"] = bool(r["lost"])
        return r


class HeaderDecoder(_Handle):
    """The header blocks of one transport decoded on the device (grdma_h2_hpack): the HPACK blocks of the parser's
    deframings as a block table, a field table and a string arena in device memory.  One per parser; independent of
    FlowControl, SendWindows and ControlReplies, which may consume the same deframing."""

    KIND, WHAT = "hpack", "h2 header decoder"  # grdma_h2_hpack_create, grdma_h2_hpack_destroy
    RESULT = ("blocks", "fields", "string_bytes", "inserted", "evicted", "table_bytes", "flags", "overflow")
    STATS = ("calls", "blocks", "fields", "string_bytes", "inserted", "evicted", "flags", "kernel_us")
    FAILED, LOST, OPEN = 1, 2, 4
    ERRORS = (None, "padding", "block too large", "integer", "truncated", "huffman", "index", "size update", "deframer")

    def __init__(self, parser, max_table_size=4096, max_block_bytes=65536):
        self.parser = parser  # (kept alive)
        self._create(parser.h, max_table_size, max_block_bytes)

    def set_max_table_size(self, n):
        """our SETTINGS_HEADER_TABLE_SIZE from now on: the bound of the peer's size updates; a lowered one evicts at once"""
        check(self.lib.grdma_h2_hpack_set_max_table_size(self.h, n))

    def decode(self, blocks_ptr, blocks_cap, fields_ptr, fields_cap, strings_ptr, strings_cap):
        """decodes the header blocks of the parser's last standalone deframing into the three device targets -> (block
        count, result tuple (RESULT)); raises GrdmaError on a refusal, a lost call or a capacity overflow -- the result
        of the failed call stays in .last_result; after a capacity overflow (overflow word 1) the call may be repeated
        with larger targets.  flags: FAILED | LOST | OPEN, the error in bits 8..15, the failing stream from bit 32"""
        n = self._call("decode", blocks_ptr, blocks_cap, fields_ptr, fields_cap, strings_ptr, strings_cap)  # grdma_h2_hpack_decode
        return n, self.last_result

    def table(self):
        """the live dynamic table -> ([(name, value), ...] newest first, (entries, table bytes, the size limit in force))"""
        return _table_dump(self.lib.grdma_h2_hpack_table, self.h)

    def stats(self):
        """dict of STATS; `flags`: the sticky word (FAILED | LOST, error << 8, stream << 32)"""
        return self._stats()  # grdma_h2_hpack_stats


def _table_dump(call, h):
    """a dynamic table through grdma_h2_hpack_table / grdma_h2_hpenc_table -> ([(name, value)] newest first, (entries,
    table bytes, the size limit in force))"""
    out = (u64 * 4)()
    rc = call(h, None, 0, out)
    if rc and not out[1]:
        check(rc)
    buf = C.create_string_buffer(max(1, int(out[1])))
    check(call(h, buf, int(out[1]), out))
    raw, pos, entries = buf.raw, 0, []
    for _ in range(int(out[0])):
        nl, vl = int.from_bytes(raw[pos:pos + 4], "little"), int.from_bytes(raw[pos + 4:pos + 8], "little")
        entries.append((raw[pos + 8:pos + 8 + nl], raw[pos + 8 + nl:pos + 8 + nl + vl]))
        pos += 8 + nl + vl
    return entries, (int(out[0]), int(out[2]), int(out[3]))


class HeaderEncoder(_Handle):
    """Header lists encoded on the device (grdma_h2_hpenc): a block table, a field table and a string arena in device
    memory -- the layout HeaderDecoder writes -- into the wire bytes of HEADERS and CONTINUATION frames, against the
    peer's dynamic table.  One per connection; it follows no parser."""

    KIND, WHAT = "hpenc", "h2 header encoder"  # grdma_h2_hpenc_create, grdma_h2_hpenc_destroy
    RESULT = ("blocks", "frames", "wire_bytes", "inserted", "evicted", "table_bytes", "flags", "overflow")
    STATS = ("calls", "blocks", "fields", "list_bytes", "wire_bytes", "inserted", "evicted", "kernel_us")
    BAD_INPUT = 1
    ERRORS = (None, "field range", "stream", "length", "string", "block too large")

    def __init__(self, peer_table_size=4096, peer_max_frame=16384):
        self._create(peer_table_size, peer_max_frame)

    def set_peer(self, peer_table_size, peer_max_frame):
        """the peer's SETTINGS_HEADER_TABLE_SIZE and SETTINGS_MAX_FRAME_SIZE from now on; the next call that sends a block
        opens it with the size update(s)"""
        check(self.lib.grdma_h2_hpenc_set_peer(self.h, peer_table_size, peer_max_frame))

    def encode(self, blocks_ptr, nblocks, fields_ptr, nfields, strings_ptr, strings_bytes, wire_ptr, wire_cap, block_wire_ptr, block_wire_cap):
        """-> (frame count, result tuple (RESULT)); raises GrdmaError on a refusal, on bad input (flags: BAD_INPUT | error
        << 8 | block << 32) and on a capacity overflow (overflow word 1: nothing was written or committed, the call may
        be repeated with larger targets) -- the result of the failed call stays in .last_result"""
        self.last_result = None
        n = self._call("encode", blocks_ptr, nblocks, fields_ptr, nfields, strings_ptr, strings_bytes, wire_ptr, wire_cap, block_wire_ptr,
                       block_wire_cap)  # grdma_h2_hpenc_encode
        return n, self.last_result

    def table(self):
        """the encoder's view of the peer's dynamic table, as HeaderDecoder.table"""
        return _table_dump(self.lib.grdma_h2_hpenc_table, self.h)

    def stats(self):
        return self._stats()  # grdma_h2_hpenc_stats

    def last_stages(self):
        """the last call's kernel time by stage, microseconds: (scan, walk, emit and commit, total)"""
        out = (u64 * 4)()
        check(self.lib.grdma_h2_hpenc_last_stages(self.h, out))
        return tuple(int(x) / 1e3 for x in out)


_CALL_META_FIELDS = ("stream", "word", "method", "http_status", "grpc_status", "timeout_lo", "timeout_hi", "path_field",
                     "authority_field", "message_field", "ncustom", "bad_field")  # grdma_h2_call_meta: twelve 32-bit words


# grdma_h2_meta_item: ten 64-bit words, the arguments of CallMetadata.read in order
META_ITEM = ("d_blocks", "nblocks", "d_fields", "nfields", "d_strings", "strings_bytes", "d_meta", "meta_cap", "d_reject", "reject_cap")


def _call_meta_dtype():
    import numpy as np  # (only the call records need it)
    return np.dtype([(name, "<u4") for name in _CALL_META_FIELDS])


_CALLS_DTYPES = {
    # grdma_h2_dispatch (48 bytes), grdma_h2_call_done (32), grdma_h2_call_entry (48)
    "DISPATCH": [("offset", "<u8"), ("length", "<u8"), ("call", "<u8"), ("stream", "<u4"), ("msg", "<u4"), ("method", "<u4"), ("word", "<u4"),
                 ("seq", "<u4"), ("pad", "<u4")],
    "CALL_DONE": [("call", "<u8"), ("bytes", "<u8"), ("stream", "<u4"), ("method", "<u4"), ("messages", "<u4"), ("word", "<u4")],
    "CALL_ENTRY": [("call", "<u8"), ("deadline_ns", "<u8"), ("bytes", "<u8"), ("stream", "<u4"), ("method", "<u4"), ("messages", "<u4"),
                   ("word", "<u4"), ("pad0", "<u4"), ("pad1", "<u4")],
}


def __getattr__(name):
    if name == "CALL_META":  # the numpy structured dtype of grdma_h2_call_meta (48 bytes), made on first use
        return _call_meta_dtype()
    if name in _CALLS_DTYPES:  # the call table's records, as numpy structured dtypes
        import numpy as np
        return np.dtype(_CALLS_DTYPES[name])
    raise AttributeError(name)


class CallMetadata(_Handle):
    """gRPC's reading of decoded header blocks on the device (grdma_h2_meta): a block table, a field table and a string
    arena in device memory -- the layout HeaderDecoder writes -- into one call record per block (CALL_META) and a compact
    list of rejection blocks over the reader's constant tables, which HeaderEncoder.encode takes as they are.  Stateless
    between calls apart from its counters; it follows no parser."""

    KIND, WHAT = "meta", "h2 metadata reader"  # grdma_h2_meta_create, grdma_h2_meta_destroy
    RESULT = ("blocks", "requests", "responses", "trailers", "rejections", "malformed", "flags", "overflow")
    STATS = ("calls", "blocks", "requests", "responses", "trailers", "rejections", "malformed", "kernel_us")
    NONE = 0xffffffff
    REQUEST, RESPONSE, TRAILERS = 1, 2, 3  # kind: word bits 0..7
    (OK, MALFORMED, BAD_METHOD, BAD_CONTENT_TYPE, BAD_TE, BAD_TIMEOUT, UNIMPLEMENTED, BAD_ENCODING, HTTP_STATUS, NO_STATUS,
     BAD_GRPC_STATUS) = range(11)  # verdict: word bits 8..15
    HAS_TIMEOUT, END_STREAM, HAS_GRPC_STATUS, HAS_MESSAGE = 1, 2, 4, 8  # flags: word bits 24..31
    ENCODINGS = ("identity", "gzip", "deflate")  # bit k of accept_encodings; encoding k in word bits 16..23, 255: another
    BAD_INPUT = 1
    ERRORS = (None, "field range", "stream", "string")
    last_results = None  # of the last read_batch

    def __init__(self, methods=(), accept=("identity",)):
        methods = [bytes(m) for m in methods]
        dump = b"".join(len(m).to_bytes(4, "little") + m for m in methods)
        bits = 0
        for name in accept:
            bits |= 1 << self.ENCODINGS.index(name)
        self._create(dump, len(dump), len(methods), bits)

    def read(self, blocks_ptr, nblocks, fields_ptr, nfields, strings_ptr, strings_bytes, meta_ptr, meta_cap, reject_ptr, reject_cap):
        """-> (rejection blocks, result tuple (RESULT)); raises GrdmaError on a refusal, on bad input (flags: BAD_INPUT |
        error << 8 | block << 32) and on a capacity overflow (overflow word 1: nothing was written, no counter moved, the
        call may be repeated with larger targets) -- the result of the failed call stays in .last_result"""
        self.last_result = None
        n = self._call("read", blocks_ptr, nblocks, fields_ptr, nfields, strings_ptr, strings_bytes, meta_ptr, meta_cap, reject_ptr,
                       reject_cap)  # grdma_h2_meta_read
        return n, self.last_result

    def read_batch(self, items):
        """CallMetadata.read for many links in three launches through this ONE reader (grdma_h2_meta_read_batch).  items:
        [(blocks device ptr, nblocks, fields device ptr, nfields, strings device ptr, strings bytes, record-table device
        ptr, record cap, rejection-list device ptr, rejection cap), ...], the ten arguments of read (META_ITEM names
        them); input tables may be shared between items, targets may not.  -> (the number of items read, [result tuple
        (RESULT) per item]); an item with bad input or a cap overflow reports for itself in its tuple (flags: BAD_INPUT |
        error << 8 | block << 32, the other words 0; overflow word 1 and the totals: nothing of it was written and it may
        be repeated, alone or in a later batch).  The counters move by ONE call and by the sums over the items read; by
        nothing where no item was read.  The result tuples also stay in .last_results, before a failure raises.  Raises
        GrdmaError only on a refusal of the whole call (the library leaves the result words alone: all 0)."""
        import numpy as np
        self.last_results = None
        arr = np.zeros((max(1, len(items)), len(META_ITEM)), dtype="<u8")  # grdma_h2_meta_item: ten 64-bit words
        for row, item in zip(arr, items):
            row[:] = [int(v or 0) for v in item]
        out = (u64 * (8 * max(1, len(items))))()
        rc = self.lib.grdma_h2_meta_read_batch(self.h, arr.ctypes.data_as(C.c_void_p), len(items), out)
        self.last_results = [tuple(int(x) for x in out[8 * i:8 * i + 8]) for i in range(len(items))]
        return check(rc), self.last_results

    def reject_tables(self):
        """the constant tables the rejection blocks point into -> (fields device ptr, fields, strings device ptr, string
        bytes): the field table and the string arena of a HeaderEncoder.encode of the rejection list"""
        out = (u64 * 4)()
        check(self.lib.grdma_h2_meta_reject_tables(self.h, out))
        return tuple(int(x) for x in out)

    def stats(self):
        return self._stats()  # grdma_h2_meta_stats

    @staticmethod
    def records(raw_bytes):
        """the bytes of a record table as a numpy array of CALL_META (a view: no copy)"""
        import numpy as np
        return np.frombuffer(raw_bytes, dtype=_call_meta_dtype())


class CallTable(_Handle):
    """Per-call state of one connection on the device, keyed by stream (grdma_h2_calls): a step joins it with the call
    records of CallMetadata.read, the descriptors of Parser.deframe_messages and the deframer's events, all in device
    memory, and writes the messages sorted by method (DISPATCH records, nmethods + 2 segment words) and a done list
    (CALL_DONE).  It follows no parser."""

    KIND, WHAT = "calls", "h2 call table"  # grdma_h2_calls_create, grdma_h2_calls_destroy
    RESULT = ("opened", "dispatched", "orphans", "done", "expired", "live", "flags", "overflow")
    STATS = ("steps", "opened", "messages", "bytes", "orphans", "done", "lost", "kernel_us")
    NONE = 0xffffffff
    BAD_INPUT, LOST = 1, 2
    ERRORS = (None, "stream", "method")
    FIRST, LAST, COMPRESSED = 1, 2, 4  # a dispatch record's flags: word bits 0..7
    NO_CALL, EXPIRED, BAD_STATUS, COMPRESSED_IDENTITY = 1, 2, 3, 4  # an orphan's reason: word bits 8..15
    READS_CLOSED, LEFT, DEADLINE = 1, 2, 3  # a done record's reason: word bits 0..7
    WAS_READS_CLOSED = 1

    def __init__(self, table_slots=0, nmethods=0):
        self.nmethods = nmethods
        self._create(table_slots, nmethods)

    def step(self, blocks_ptr, meta_ptr, nblocks, msgs_ptr, nmsgs, events_ptr, nevents, now_ns, dispatch_ptr, dispatch_cap, segments_ptr,
             done_ptr, done_cap):
        """-> (dispatch records, result tuple (RESULT)); raises GrdmaError on a refusal, on bad input (flags: BAD_INPUT |
        error << 8 | record << 32) and on a capacity overflow (overflow word 1: nothing was written or committed, the
        step may be repeated with larger targets) -- the result of the failed step stays in .last_result"""
        self.last_result = None
        n = self._call("step", blocks_ptr, meta_ptr, nblocks, msgs_ptr, nmsgs, events_ptr, nevents, now_ns, dispatch_ptr, dispatch_cap,
                       segments_ptr, done_ptr, done_cap)  # grdma_h2_calls_step
        return n, self.last_result

    def dump(self):
        """-> (the live entries sorted by stream as a numpy array of CALL_ENTRY, (entries, the serial counter,
        table_slots))"""
        import numpy as np
        out = (u64 * 4)()
        rc = self.lib.grdma_h2_calls_dump(self.h, None, 0, out)
        if rc and not out[1]:
            check(rc)
        buf = C.create_string_buffer(max(1, int(out[1])))
        check(self.lib.grdma_h2_calls_dump(self.h, buf, int(out[1]), out))
        return np.frombuffer(buf.raw[:int(out[1])], dtype=np.dtype(_CALLS_DTYPES["CALL_ENTRY"])), (int(out[0]), int(out[2]), int(out[3]))

    def stats(self):
        return self._stats()  # grdma_h2_calls_stats


# grdma_h2_calls_item: fourteen 64-bit words, the table and the arguments of CallTable.step in order
CALLS_ITEM = ("calls", "d_blocks", "d_meta", "nblocks", "d_msgs", "nmsgs", "d_events", "nevents", "now_ns", "d_dispatch", "dispatch_cap",
              "d_segments", "d_done", "done_cap")


def calls_step_batch(items):
    """CallTable.step for the tables of many connections in eight launches (grdma_h2_calls_step_batch).  items:
    [(CallTable, blocks device ptr, record-table device ptr, nblocks, descriptors device ptr, nmsgs, events device ptr,
    nevents, now_ns, dispatch device ptr, dispatch cap, segments device ptr, done-list device ptr, done cap), ...] with
    distinct tables (CALLS_ITEM names the columns); input tables may be shared between items, targets may not.  -> (the
    number of items that committed, [result tuple (CallTable.RESULT) per item]); an item with bad input or a cap overflow
    reports for itself in its tuple (flags: BAD_INPUT | error << 8 | record << 32, the other words 0; overflow word 1 and
    the totals: nothing of it was written or committed and it may be repeated, alone or in a later batch).  The result
    tuples also land in each table's .last_result, before a failure raises.  Raises GrdmaError only on a refusal of the
    whole call (the library leaves the result words alone: all 0)."""
    import numpy as np
    arr = np.zeros((max(1, len(items)), len(CALLS_ITEM)), dtype="<u8")  # grdma_h2_calls_item: fourteen 64-bit words
    for row, item in zip(arr, items):
        row[0] = int(item[0].h or 0) if item[0] is not None else 0
        row[1:] = [int(v or 0) for v in item[1:]]
    out = (u64 * (8 * max(1, len(items))))()
    rc = load().grdma_h2_calls_step_batch(arr.ctypes.data_as(C.c_void_p), len(items), out)
    results = [tuple(int(x) for x in out[8 * i:8 * i + 8]) for i in range(len(items))]
    for item, r in zip(items, results):
        if item[0] is not None:  # (an item without table: the whole call is refused below)
            item[0].last_result = r
    return check(rc), results


def decode_batch(items):
    """HeaderDecoder.decode for many transports in six launches (grdma_h2_hpack_decode_batch).  items: [(HeaderDecoder,
    blocks device ptr, blocks cap, fields device ptr, fields cap, strings device ptr, strings cap), ...] with distinct
    decoders; each decodes the last standalone deframing of its own parser into its own targets.  -> (the number of items
    without overflow, [result tuple (HeaderDecoder.RESULT) per item]); an item whose call was lost or overflowed a cap
    reports for itself in its tuple (overflow word 2 / 1: after 1 nothing of it was written or committed and it may be
    repeated, alone or in a later batch).  The result tuples also land in each decoder's .last_result.  Raises
    GrdmaError only on a refusal."""
    return _batch(load().grdma_h2_hpack_decode_batch, _items(H2HpackItem, items), items)


def encode_batch(items):
    """HeaderEncoder.encode for many connections in four launches (grdma_h2_hpenc_encode_batch).  items: [(HeaderEncoder,
    blocks device ptr, nblocks, fields device ptr, nfields, strings device ptr, strings bytes, wire device ptr, wire cap,
    block-wire device ptr, block-wire cap), ...] with distinct encoders; each encodes its own input (input tables may be
    shared between items) against its own peer table into its own targets.  -> (the number of items whose blocks are on
    the wire, [result tuple (HeaderEncoder.RESULT) per item]); an item with bad input or a cap overflow reports for itself
    in its tuple (flags: BAD_INPUT | error << 8 | block << 32; overflow word 1: nothing of it was written or committed
    and it may be repeated, alone or in a later batch).  The result tuples also land in each encoder's .last_result.
    Raises GrdmaError only on a refusal of the whole call."""
    return _batch(load().grdma_h2_hpenc_encode_batch, _items(H2HpencItem, items), items)


def control_batch(items):
    """ControlReplies.reply for many transports in four launches (grdma_h2_ctl_reply_batch).  items: [(ControlReplies,
    slices device ptr, slices cap, header arena device ptr, header cap), ...] with distinct writers; each answers the last
    standalone deframing of its own parser.  -> per item ([(ptr, len), ...], result tuple (ControlReplies.RESULT)); an
    item whose call was lost or overflowed a cap reports for itself: its result tuple and None, nothing of it was
    written.  The result tuples also land in each writer's .last_result.  Raises GrdmaError on a refusal."""
    lib = load()
    _, results = _batch(lib.grdma_h2_ctl_reply_batch, _items(H2CtlItem, items), items)
    return [(r, None) if r[7] else (_read_slice_table(lib, item[1], r[1]), r) for item, r in zip(items, results)]


def account_batch(items):
    """FlowControl.account for many transports in five launches (grdma_h2_fc_account_batch).  items: [(FlowControl,
    slices device ptr, slices cap, header arena device ptr, header cap), ...] with distinct, unattached ledgers; each
    accounts the last standalone deframing of its own parser.  -> per item ([(ptr, len), ...], result tuple
    (FlowControl.RESULT), wire bytes); an item whose call was lost or overflowed a cap reports for itself: its result
    tuple and None, nothing of it was written.  The result tuples also land in each ledger's .last_result."""
    lib = load()
    _, results = _batch(lib.grdma_h2_fc_account_batch, _items(H2FcItem, items), items)
    res = []
    for item, r in zip(items, results):
        if r[7]:
            res.append((r, None))
            continue
        sl = _read_slice_table(lib, item[1], r[1])
        res.append((sl, r, _read_wire(lib, sl)))
    return res


def intake_batch(sws):
    """SendWindows.intake for many transports in three launches (grdma_h2_sw_intake_batch).  sws: distinct SendWindows;
    each takes in the last standalone deframing of its own parser.  -> per item its result tuple (SendWindows.INTAKE);
    an item whose call was lost reports for itself (overflow word 2, the LOST bit): its tuple is in the list, the
    others are exact.  The result tuples also land in each object's .last_result.  Raises GrdmaError on a refusal."""
    arr = (C.c_void_p * max(1, len(sws)))(*[s.h if s is not None else None for s in sws])
    return _batch(load().grdma_h2_sw_intake_batch, arr, [(s,) for s in sws])[1]


def frame_windowed_batch(items):
    """SendWindows.frame for many transports in two launches (grdma_h2_sw_frame_batch).  items: [(SendWindows, msgs,
    progress, max_frame, slices device ptr, slices cap, header arena device ptr, header cap), ...] with distinct send
    windows, msgs and progress as SendWindows.frame takes them.  -> per item ([(ptr, len), ...], result tuple
    (SendWindows.FRAME), progress after the call); an item whose cap overflowed reports for itself: its result tuple and
    None -- nothing of it was written, no window of it moved.  The result tuples also land in each object's
    .last_result.  Raises GrdmaError on a refusal."""
    lib = load()
    rows = []  # (per item the struct's fields in their order, arrays for msgs and progress; they also keep the arrays alive)
    for sw, msgs, progress, max_frame, *target in items:
        marr = _msg_array(msgs) if msgs is not None else None
        prog = (u64 * max(1, len(progress)))(*progress) if progress is not None else None
        rows.append((sw, marr, prog, len(msgs) if msgs is not None else 0, max_frame, 0, *target))
    _, results = _batch(lib.grdma_h2_sw_frame_batch, _items(H2SwFrameItem, rows), items)
    return [(r, None) if r[7] else (_read_slice_table(lib, item[4], r[2]), r, [int(x) for x in row[2][:len(item[1])]])
            for item, row, r in zip(items, rows, results)]


class Pipe:
    """frame -> streaming job -> deframe as one enqueued device pipeline (grdma_h2_pipe).
    msgs: list of (payload device ptr, len, stream_id, flags); the job must have been run once.
    link: the one link of the job this pipe serves.  A job carries one pipe: for more than one link of one job use
    GroupPipe (a second Pipe on another link would replace this one's kernels in the job's graph)."""

    def __init__(self, job, msgs, parser, delivered_slices, events_cap, link=0, max_frame=16384):
        self.lib = load()
        self.events_cap = events_cap
        self.delivered = delivered_slices
        self.parser = parser  # (kept alive)
        self.h = self.lib.grdma_h2_pipe_create(job.h, link, _msg_array(msgs), len(msgs), max_frame, parser.h, delivered_slices,
                                               events_cap)
        if not self.h:
            raise GrdmaError("h2 pipe allocation failed")

    @classmethod
    def reply(cls, job, reply, parser, delivered_slices, events_cap, recorded_wire_bytes, link=0):
        """A pipe whose framing stage is `reply` (grdma_h2_pipe_create_reply): a step frames what the last enqueued
        forward step reported, sends it through `job` and deframes it with `parser`.  recorded_wire_bytes: what the
        job's recorded run sent.  Close it before the forward pipes and before `reply`."""
        self = cls.__new__(cls)
        self.lib = load()
        self.events_cap = events_cap
        self.delivered = delivered_slices
        self.parser, self.reply_framer = parser, reply  # (kept alive)
        self.h = self.lib.grdma_h2_pipe_create_reply(job.h, link, reply.h, parser.h, delivered_slices, events_cap,
                                                     recorded_wire_bytes)
        if not self.h:
            raise GrdmaError("h2 reply pipe creation failed")
        reply.assembler._reply_pipes = getattr(reply.assembler, "_reply_pipes", 0) + 1
        return self

    def slice_table(self, cap=1 << 16):
        """the slice table the job sends from, [(ptr, len), ...], once the enqueued steps have ended"""
        arr = (Slice * cap)()
        n = check(self.lib.grdma_h2_pipe_slice_table(self.h, arr, cap))
        return [(int(arr[i].ptr or 0), int(arr[i].len)) for i in range(n)]

    def enqueue(self, _unused=False):
        check(self.lib.grdma_h2_pipe_enqueue(self.h, 0))

    def sync(self, want_events=False):
        """-> dict(framed, frame_overflow, events, deframe_overflow, parsed, h2_error[, event list])"""
        out = (u64 * 14)()
        ev = (H2Event * self.events_cap)() if want_events else None
        check(self.lib.grdma_h2_pipe_sync(self.h, out, ev, self.events_cap if want_events else 0))
        r = dict(zip(SYNC_KEYS, [int(x) for x in out]))
        bs = (u64 * 2)()
        check(self.lib.grdma_h2_pipe_boundary_stats(self.h, bs))
        r["boundary_steps"], r["t_boundary"] = int(bs[0]), int(bs[1])
        if want_events:
            r["event_list"] = _events(ev, min(r["events"], self.events_cap))
        return r

    def attach_assembler(self, a):
        check(self.lib.grdma_h2_pipe_attach_assembler(self.h, a.h))
        self.assembler = a  # (kept alive)

    def messages(self, cap=None):
        """the messages of the last synced step"""
        cap = cap or self.events_cap
        out = (H2RxMsg * cap)()
        m = check(self.lib.grdma_h2_pipe_messages(self.h, out, cap))
        return _msgs(out, m)

    def attach_flow_control(self, fc):
        """every step accounts its events through the ledger fc (grdma_h2_pipe_attach_flow_control)"""
        check(self.lib.grdma_h2_pipe_attach_flow_control(self.h, fc.h))
        self.flow_control = fc  # (kept alive)
        fc._pipe = self

    def window_updates(self):
        """the window-update list of the last step -> ([(ptr, len), ...], result tuple, wire bytes)"""
        fc = self.flow_control
        cap = (13 * fc.max_updates + 22) // 23
        arr = (Slice * max(1, cap))()
        out = (u64 * 8)()
        n = self.lib.grdma_h2_pipe_window_updates(self.h, arr, cap, out)
        res = tuple(int(x) for x in out)
        n = check(n)
        buf = C.create_string_buffer(max(1, res[2]))
        m = check(self.lib.grdma_h2_pipe_window_update_bytes(self.h, buf, res[2]))
        return [(int(arr[i].ptr or 0), int(arr[i].len)) for i in range(n)], res, buf.raw[:m]

    def close(self):
        if self.h:
            a = getattr(self, "assembler", None)
            if a is not None and getattr(a, "_reply_pipes", 0):
                # (grdma_h2_pipe_destroy does nothing then: a reply pipe's job gathers from this pipe's arena)
                raise GrdmaError("close the reply pipe that reads this pipe's assembler first")
            self.lib.grdma_h2_pipe_destroy(self.h)
            self.h = None
            fc = getattr(self, "flow_control", None)
            if fc is not None:
                fc._pipe = None
            rf = getattr(self, "reply_framer", None)
            if rf is not None:
                rf.assembler._reply_pipes -= 1
