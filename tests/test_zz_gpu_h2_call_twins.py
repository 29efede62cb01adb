"""The single call and the batch call of a facility are the same per-item steps (csrc/grdma_h2_host_calls.inc): for the
ledger's account, the send windows' intake and framing, the control replies and the windowed reply, every refusal that
can be reached from here makes the single call and a batch of ONE item fail with the same error code and leaves the
object as it was (the valid call still runs behind it), and a valid single call and a valid batch of one, on two
transports fed the same bytes, give equal result words and equal output bytes.  Every refusal is found on the host in
front of any launch.  The input is the smallest that walks the paths: one delivered slice of a 9-byte SETTINGS frame, a
13-byte WINDOW_UPDATE and a 1-byte DATA frame on stream 1, 16 table slots, 8 events, targets of 8 slices and 256 header
bytes."""
import re

import pytest

from tests.h2_device_lib import ERR_INVALID, SENTINEL, device_bytes, pack_slices
from tests.h2_helpers import frame
from tests.h2_send_lib import window_update

pytestmark = pytest.mark.gpu

WIRE = frame(4, 0, 0) + window_update(0, 5) + frame(0, 0, 1, b"x")
assert len(WIRE) == 9 + 13 + 10
EV_CAP, SLICES, HDR = 8, 8, 256


class Link:
    """One transport: a parser with stream 1 open, the delivered slice in device memory, a target, and the facility's
    object(s) as make(link) creates them."""

    def __init__(self, g, make):
        from grpc_rdma_amd import h2dev
        self.g, self.h2dev = g, h2dev
        self.parser = h2dev.Parser(False, table_slots=16)
        assert self.parser.open_streams([1]) == 0
        data, self.table = pack_slices([WIRE])
        self.buf = g.DeviceBuffer(data=data)
        self.t = g.DeviceBuffer(data=bytes([SENTINEL]) * 1024)
        self.pay = g.DeviceBuffer(data=b"y" + bytes(15))
        self.target = (self.t.ptr, SLICES, self.t.ptr + 256, HDR)
        self.asm = self.reply = None
        make(self)

    def deframe(self):
        if self.asm is not None:
            assert self.parser.deframe_messages(self.buf.ptr, self.table, self.asm, ev_cap=EV_CAP)[0] == 0
        else:
            assert self.parser.deframe(self.buf.ptr, self.table, cap=EV_CAP)[0] == 0

    def with_reply(self, attach):
        """an assembler and a reply framer on the parser; attach: the reply frames under self.sw"""
        self.arena = self.g.DeviceBuffer(nbytes=4096)
        self.asm = self.h2dev.Assembler(self.parser, self.arena, 1 << 20, 8)
        self.reply = self.h2dev.Reply(self.asm, None, 16384, 8)
        if attach:
            self.reply.attach_windows(self.sw, 8)

    def wire(self, slices):
        return b"".join(device_bytes(self.g, ptr, n) for ptr, n in slices)


def bad_targets(link):
    sl, cap, hdr, hdr_cap = link.target
    return (("null slice table", (0, cap, hdr, hdr_cap)), ("null header arena", (sl, cap, 0, hdr_cap)),
            ("zero slices", (sl, 0, hdr, hdr_cap)), ("zero header bytes", (sl, cap, hdr, 0)),
            ("misaligned slice table", (sl + 8, cap, hdr, hdr_cap)), ("misaligned header arena", (sl, cap, hdr + 4, hdr_cap)))


# ---- the facilities: make(link), single(link, target), batch(link, target) -> (result words, output bytes) ---------------
MSG = lambda link: [(link.pay.ptr, 1, 1, 0)]  # noqa: E731  (one 1-byte message on stream 1)


def make_fc(link):
    link.fc = link.h2dev.FlowControl(link.parser, max_updates=8)


def fc_single(link, target):
    sl, res, wire = link.fc.account(*target)
    return res + tuple(n for _, n in sl), wire


def fc_batch(link, target):
    (sl, res, wire), = link.h2dev.account_batch([(link.fc,) + tuple(target)])
    return res + tuple(n for _, n in sl), wire


def make_sw(link):
    link.sw = link.h2dev.SendWindows(link.parser)


def intake_single(link, target):
    return link.sw.intake(), b""


def intake_batch(link, target):
    return link.h2dev.intake_batch([link.sw])[0], b""


def frame_single(link, target, msgs=None, progress=(0,)):
    sl, res, prog = link.sw.frame(MSG(link) if msgs is None else msgs, list(progress), 16384, *target)
    return res + tuple(prog), link.wire(sl)


def frame_batch(link, target, msgs=None, progress=(0,)):
    (sl, res, prog), = link.h2dev.frame_windowed_batch([(link.sw, MSG(link) if msgs is None else msgs, list(progress), 16384) + tuple(target)])
    return res + tuple(prog), link.wire(sl)


def make_ctl(link):
    link.ctl = link.h2dev.ControlReplies(link.parser, 8)


def ctl_single(link, target):
    sl, res = link.ctl.reply(*target)
    return res, link.wire(sl)


def ctl_batch(link, target):
    (sl, res), = link.h2dev.control_batch([(link.ctl,) + tuple(target)])
    return res, link.wire(sl)


def make_wr(link):
    make_sw(link)
    link.with_reply(attach=True)


def _windowed(link, sl, st):
    st = dict(st, frame_us=0)   # (a time)
    return tuple(st[k] for k in link.h2dev.Reply.WINDOWED), link.wire(sl)


def wr_single(link, target):
    return _windowed(link, *link.reply.frame_windowed(*target))


def wr_batch(link, target):
    (sl, st), = link.h2dev.reply_frame_windowed_batch([(link.reply,) + tuple(target) + (False,)])
    assert not isinstance(sl, int), sl
    return _windowed(link, sl, st)


FACILITIES = {
    "ledger-account": (make_fc, fc_single, fc_batch),
    "send-window-intake": (make_sw, intake_single, intake_batch),
    "send-window-frame": (make_sw, frame_single, frame_batch),
    "control-reply": (make_ctl, ctl_single, ctl_batch),
    "windowed-reply": (make_wr, wr_single, wr_batch),
}
FOLLOWERS = ("ledger-account", "send-window-intake", "control-reply")   # (each takes a standalone deframing once)
TARGETED = ("ledger-account", "send-window-frame", "control-reply", "windowed-reply")


def code(g, call, *args, **kw):
    """the error code the call fails with, 0 when it runs"""
    try:
        call(*args, **kw)
    except g.GrdmaError as e:
        return int(re.match(r"grdma error (\d+)", str(e)).group(1))
    return 0


@pytest.mark.parametrize("name", sorted(FACILITIES))
def test_refusals_have_one_code_and_change_nothing(gpu, name):
    g = gpu
    make, single, batch = FACILITIES[name]
    link = Link(g, make)

    def refused(what, *args, **kw):
        got = code(g, single, link, *args, **kw), code(g, batch, link, *args, **kw)
        assert got == (ERR_INVALID, ERR_INVALID), (name, what, got)

    def valid(call):
        res, _ = call(link, link.target)
        assert res[7] == 0, (name, res)   # (the overflow word of every result block)

    if name in FOLLOWERS or name == "windowed-reply":
        refused("nothing deframed yet", link.target)
    link.deframe()
    if name in TARGETED:
        for what, target in bad_targets(link):
            refused(what, target)
    if name == "send-window-frame":
        refused("no message", link.target, msgs=[], progress=[])
        refused("too many messages", link.target, msgs=MSG(link) * 4097, progress=[0] * 4097)
        refused("a finished message", link.target, progress=[6])
    valid(batch)   # (behind the refused batches of one)
    if name in FOLLOWERS:
        refused("taken already", link.target)
        link.deframe()
    valid(single)
    link.deframe()
    # what an object outlives: the reply framer whose queue waited under the send windows, the send windows, the parser
    if name.startswith("send-window"):
        gone = Link(g, make)
        gone.with_reply(attach=True)
        gone.deframe()
        gone.reply.close()
        link, keep = gone, link
        refused("reply gone", link.target)
        link = keep
    if name == "windowed-reply":
        gone = Link(g, make)
        gone.deframe()
        gone.sw.close()
        link, keep = gone, link
        refused("send windows gone", link.target)
        link = keep
    link.parser.close()
    refused("parser gone", link.target)


@pytest.mark.parametrize("name", sorted(FACILITIES))
def test_a_batch_of_one_is_the_single_call(gpu, name):
    make, single, batch = FACILITIES[name]
    a, b = Link(gpu, make), Link(gpu, make)
    for link in (a, b):
        link.deframe()
    one, many = single(a, a.target), batch(b, b.target)
    assert one == many, (name, one, many)
    assert one[0][7] == 0
    if name in ("ledger-account", "send-window-frame", "control-reply"):
        assert one[1], name   # (a WINDOW_UPDATE for the DATA byte, the framed message, the SETTINGS ACK)
