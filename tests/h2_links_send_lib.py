"""The harness of the many-link send flow control device tests (tests/test_zz_gpu_h2_links_send_window.py): a list of SH
harnesses (tests/h2_send_lib.py: a device parser with its send windows, the oracle's parser and a SendModel each) under
the two batch calls.  Every item of a batch is compared exactly with its own link's model: result words, windows,
counters, progress, slice tables, wire images.  pytest rewrites no `assert` in a helper module, so every check here goes
through `same`."""
import ctypes as C

from oracle import pyorc
from tests.h2_device_lib import SENTINEL, read_slices, same
from tests.h2_flow_model import Model as LedgerModel
from tests.h2_send_lib import window_update
from tests.h2_send_model import SendModel


def deframe_all(hs, calls, ev_cap=None):
    """one standalone deframing per link: calls[i] is link i's slice list (None: the link sits this round out)"""
    for h, slices in zip(hs, calls):
        if slices is not None:
            h.deframe(slices, ev_cap)


def intake_batch(hs, order, lost=(), got=None):
    """one h2dev.intake_batch over the links listed in `order`, every item against its model -> {link: result}.
    lost: links whose last deframing overflowed its event list; got: the result tuples of a call made elsewhere
    (intake_batch_raw), compared in place of a call"""
    h2dev = hs[order[0]].h2dev
    mirrored = got is None
    if mirrored:
        got = h2dev.intake_batch([hs[i].sw for i in order])
    same(len(got), len(order), "intake_batch: items")
    out = {}
    for k, i in enumerate(order):
        h = hs[i]
        if i in lost:
            res = h.model.lost_call()
        else:
            err_o, ev_o = h.last
            res = h.model.intake(ev_o, h.last_slices, err_o, h.live())
        print("link %d intake: %r -> %r" % (i, res, got[k]))
        same(got[k], res, "link %d: intake result" % i)
        if mirrored:
            same(h.sw.last_result, res, "link %d: .last_result" % i)
        h.check()
        out[i] = res
    return out


def intake_batch_raw(hs, order):
    """grdma_h2_sw_intake_batch itself -> (its return value, the result tuples)"""
    lib = hs[order[0]].h2dev.load()
    arr = (C.c_void_p * len(order))(*[hs[i].sw.h for i in order])
    out = (C.c_uint64 * (8 * len(order)))()
    rc = lib.grdma_h2_sw_intake_batch(arr, len(order), out)
    return rc, [tuple(int(x) for x in out[8 * k:8 * k + 8]) for k in range(len(order))]


def place(h, sl):
    """a slice list with its pointers made relative: ('h', offset in the header arena) or ('p', offset in the payloads)"""
    out = []
    for ptr, n in sl:
        if h.hdr.ptr <= ptr < h.hdr.ptr + h.hdr.nbytes:
            out.append(("h", ptr - h.hdr.ptr, n))
        else:
            out.append(("p", ptr - h.pay.ptr, n))
    return out


def frame_batch(hs, order, calls):
    """one h2dev.frame_windowed_batch over the links listed in `order`; calls[i] = (msgs, progress, max_frame[, cap[,
    hdr_cap]]) with msgs as SH.frame takes them.  Every item against its model -> {link: (lens, wire, result, progress)};
    the device's slice list of a framed link stays in hs[i].last_sl"""
    h2dev = hs[order[0]].h2dev
    items, exp = [], {}
    for i in order:
        h = hs[i]
        msgs, progress, mf = calls[i][:3]
        cap = calls[i][3] if len(calls[i]) > 3 else h.cap
        hdr_cap = calls[i][4] if len(calls[i]) > 4 else 32 * cap
        h.named |= {s for _, s, _ in msgs}
        table = h.upload_bodies(msgs)
        h.new_target(max(cap, 1))
        exp[i] = h.model.frame(msgs, progress, mf, cap, hdr_cap, h.live())
        items.append((h.sw, table, list(progress), mf, h.slices.ptr, cap, h.hdr.ptr, hdr_cap))
    got = h2dev.frame_windowed_batch(items)
    same(len(got), len(order), "frame_windowed_batch: items")
    for k, i in enumerate(order):
        h = hs[i]
        lens, wire, res, prog = exp[i]
        what = "link %d frame: " % i
        print("link %d frame: %r -> %r" % (i, res, got[k][0] if res[7] else got[k][1]))
        if res[7]:
            same(got[k], (res, None), what + "what an overflowing item hands back")
            same(h.sw.last_result, res, what + ".last_result of an overflowing item")
            same(h.slices.read(), bytes([SENTINEL]) * h.slices.nbytes, what + "slice table of an overflowing item")
            same(h.hdr.read(), bytes([SENTINEL]) * h.hdr.nbytes, what + "header arena of an overflowing item")
            h.last_sl = None
        else:
            sl, r, prog_d = got[k]
            same(r, res, what + "result")
            same(h.sw.last_result, res, what + ".last_result")
            same(prog_d, prog, what + "progress")
            same([n for _, n in sl], lens, what + "slice lengths")
            same(read_slices(h.g, h.slices, len(sl)), sl, what + "slice table")
            same(h.slices.read()[16 * len(sl):], bytes([SENTINEL]) * (h.slices.nbytes - 16 * len(sl)),
                 what + "slice table behind the last slice")
            same(h.wire_of(sl), wire, what + "wire")
            inl = [p for p, n in sl if h.hdr.ptr <= p < h.hdr.ptr + h.hdr.nbytes]
            same(inl, [h.hdr.ptr + 32 * j for j in range(len(inl))], what + "inlined slice pointers")
            same(32 * len(inl), res[3], what + "header-arena bytes")
            h.last_sl = sl
        h.check()
        h.last_frame = exp[i]
    return exp


def unfinished(msgs, prog):
    """-> (the messages with bytes left, their progress)"""
    keep = [i for i, (b, _, _) in enumerate(msgs) if prog[i] < 5 + len(b)]
    return [msgs[i] for i in keep], [prog[i] for i in keep]


def arrived(wire, streams):
    """the wire through the oracle's parser -> {stream: [message, ...]}"""
    orc = pyorc.H2Parser(False)
    for s in streams:
        same(orc.open_stream(s), 0, "oracle open_stream(%d)" % s)
    rc, ev = orc.feed(wire, cap=len(wire) + 4096)
    same(rc, 0, "the wire's h2 error")
    back, partial = {}, {}
    for k, a, b, c, d in ev:
        if k == pyorc.EV_MSG_BEGIN:
            partial[c] = bytearray()
        elif k == pyorc.EV_MSG_BYTES:
            partial[c] += wire[a:a + b]
        elif k == pyorc.EV_MSG_END:
            back.setdefault(c, []).append(bytes(partial.pop(c)))
    same(partial, {}, "messages left open")
    return back


def by_stream(msgs):
    want = {}
    for b, s, _ in msgs:
        want.setdefault(s, []).append(b)
    return want


def credit_frames(conn=0, streams=()):
    """WINDOW_UPDATE bytes for the connection and [(stream, increment)]; a PING where there is nothing to give"""
    frames = ([window_update(0, conn)] if conn else []) + [window_update(s, n) for s, n in streams if n]
    return [b"".join(frames)] if frames else [b"\x00\x00\x08\x06\x00\x00\x00\x00\x00" + bytes(8)]


def model_rounds(msgs, mf, streams=(1, 3)):
    """side A's SendModel against side B's ledger model, both fed by the oracle's parsers -> rounds until done"""
    a, b = SendModel(), LedgerModel(65535, 65535, 0, 64, streams)
    orc_a, orc_b = pyorc.H2Parser(False), pyorc.H2Parser(False)
    for s in streams:
        same((orc_a.open_stream(s), orc_b.open_stream(s)), (0, 0), "oracle open_stream(%d)" % s)
    todo, prog, rounds = list(msgs), [0] * len(msgs), 0
    while todo:
        lens, wire, res, prog = a.frame(todo, prog, mf, 1 << 20, 1 << 30, set(streams))
        todo, prog = unfinished(todo, prog)
        rc, ev = orc_b.feed(wire, cap=len(wire) + 4096)
        same(rc, 0, "model round: h2 error")
        _, res_b, back = b.call(ev, 0, 64, 32 * 64)
        same(res_b[5], 0, "model round: ledger violations")
        rc, ev = orc_a.feed(back)
        same(rc, 0, "model round: h2 error of the updates")
        a.intake([e + (0,) for e in ev], [back], 0, set(streams))
        rounds += 1
        if rounds >= 100:
            raise AssertionError("the models do not finish")
    return rounds
