"""A sequential model of the control-reply writer (grdma_h2_ctl, csrc/grdma_h2_ctl.h): rules 1 to 7 of
include/grdma_amd.h ("Control replies") applied to the ORACLE's event list (oracle/pyorc.H2Parser.feed) plus the bytes
that were fed, struct.pack for the frames and the port of the oracle's sb_add (tests/h2_send_model.py) for the slice list.
Nothing of the library's own events or output goes into it; tests/test_h2_control_model.py pins it against a byte-at-a-
time frame walker before a device test trusts it."""
from oracle.pyorc import EV_FRAME, EV_PAYLOAD
from tests.h2_send_model import sb_add

LOST, GOAWAY = 1, 2  # GRDMA_H2_CTL_*
SETTINGS, PING, GOAWAY_FRAME = 4, 6, 7
SETTINGS_ACK = bytes([0, 0, 0, 4, 1, 0, 0, 0, 0])
PEER_KEYS = ("settings_acks", "ping_acks", "last_ping_opaque", "goaways", "goaway_last_stream", "goaway_error", "goaway_call")
STAT_KEYS = ("calls", "settings_acks", "ping_acks", "rst_streams", "wire_bytes")


def ping_ack(opaque):
    return bytes([0, 0, 8, 6, 1, 0, 0, 0, 0]) + bytes(opaque)


def rst_stream(sid):
    return bytes([0, 0, 4, 3, 0]) + sid.to_bytes(4, "big") + bytes([0, 0, 0, 1])  # PROTOCOL_ERROR


def cut23(frames):
    """the slice lengths grpc_slice_buffer_add makes of these small inlined slices"""
    sb = []
    for f in frames:
        sb_add(sb, len(f), 1)
    return [n for n, _ in sb]


class ControlModel:
    def __init__(self, max_replies=4096):
        self.max_replies = max_replies
        self.carry = None  # the control frame the previous call's end cut: dict(type, flags, bytes)
        self.lost = False
        self.peer = dict.fromkeys(PEER_KEYS, 0)
        self.stats = dict.fromkeys(STAT_KEYS, 0)

    def lost_call(self):
        """a call whose event list overflowed: the flag, the carry goes, the record keeps what it knows"""
        self.lost, self.carry = True, None
        self.stats["calls"] += 1
        return [], b"", (0, 0, 0, 0, 0, 0, LOST, 2)

    def reply(self, events, slices, err, cap, hdr_cap, skipped=False):
        """events: the oracle's, tagged with the slice index; slices: the bytes fed; skipped: a standalone deframing in
        front of this one was never taken in -> (slice lengths, wire, result tuple)"""
        if err:  # nothing written, nothing recorded, taken, the carry goes
            self.lost, self.carry = self.lost or skipped, None
            self.stats["calls"] += 1
            return [], b"", (0, 0, 0, 0, 0, 0, LOST if self.lost else 0, 0)
        pings, queued, done = [], [], []  # replies, and the peer's completed frames in completion order
        n_settings = n_rst = 0
        cur = None if skipped or self.carry is None else dict(self.carry, bytes=bytearray(self.carry["bytes"]))
        for k, a, b, c, d, sl in events:
            if k == EV_FRAME:
                if a == 0xff:  # a stream error reported inside a DATA frame's payload run
                    queued.append(rst_stream(c))
                    n_rst += 1
                    continue
                cur = None
                if b >> 8:  # the status byte: a stream error
                    queued.append(rst_stream(c))
                    n_rst += 1
                elif a in (SETTINGS, PING, GOAWAY_FRAME):
                    cur = dict(type=a, flags=b & 0xff, bytes=bytearray())
            elif k == EV_PAYLOAD and cur is not None:
                if cur["type"] != SETTINGS:
                    cur["bytes"] += slices[sl][a:a + b][:8 - len(cur["bytes"])]
                if c:  # is_last: the frame's completion
                    if cur["type"] == SETTINGS and not cur["flags"] & 1:
                        queued.append(SETTINGS_ACK)
                        n_settings += 1
                    elif cur["type"] == PING and not cur["flags"] & 1:
                        pings.append(ping_ack(cur["bytes"]))
                    else:
                        done.append(cur)
                    cur = None
        frames = pings + queued  # (a fixed choice: the PING ACKs first)
        wire = b"".join(frames)
        lens = cut23(frames)
        goaways = [f for f in done if f["type"] == GOAWAY_FRAME]
        flags = (LOST if self.lost or skipped else 0) | (GOAWAY if goaways else 0)
        totals = (len(frames), len(lens), len(wire), n_settings, len(pings), n_rst, flags)
        if len(frames) > self.max_replies or len(lens) > cap or 32 * len(lens) > hdr_cap:
            return [], b"", totals + (1,)  # nothing written, nothing committed, not taken
        self.lost = self.lost or skipped
        self.carry = cur
        self.stats["calls"] += 1
        self.stats["settings_acks"] += n_settings
        self.stats["ping_acks"] += len(pings)
        self.stats["rst_streams"] += n_rst
        self.stats["wire_bytes"] += len(wire)
        for f in done:
            if f["type"] == SETTINGS:
                self.peer["settings_acks"] += 1
            elif f["type"] == PING:
                self.peer["ping_acks"] += 1
                self.peer["last_ping_opaque"] = int.from_bytes(f["bytes"], "little")
            else:
                self.peer["goaways"] += 1
                self.peer["goaway_last_stream"] = int.from_bytes(f["bytes"][:4], "big") & 0x7fffffff
                self.peer["goaway_error"] = int.from_bytes(f["bytes"][4:8], "big")
                self.peer["goaway_call"] = self.stats["calls"]
        return lens, wire, totals + (0,)
