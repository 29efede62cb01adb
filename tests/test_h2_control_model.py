"""tests/h2_control_model.py pinned before a device test trusts it: against an independent byte-at-a-time frame walker
over random streams cut into calls and slices, over the capture of a stock gRPC client, and its slice rule and frame
images against the bytes the rules give."""
import random

from oracle import pyorc
from tests.h2_control_model import (GOAWAY, ControlModel, SETTINGS_ACK, cut23, ping_ack, rst_stream)
from tests.h2_device_lib import oracle_feed
from tests.h2_helpers import PREFACE, frame, grpc_msg, grpcio_capture

STREAMS = (1, 3, 5, 7)


# ---- the walker: whole frames over the concatenated stream, a byte at a time, no events and no carry --------------------
def walk(data, streams):
    """-> [(position of the byte that makes it due, kind, value)]: kind "ping" (opaque), "settings", "rst" (stream),
    "got_settings_ack", "got_ping_ack" (opaque), "got_goaway" ((last stream, error code))"""
    out = []
    grpc = {s: dict(hdr=0, left=0, dead=False) for s in streams}  # per stream: the gRPC message parser over its DATA bytes
    closed = set()  # streams closed for reads by a stream error in a frame header
    pos = 0
    while pos < len(data):
        ln, ftype, flags = int.from_bytes(data[pos:pos + 3], "big"), data[pos + 3], data[pos + 4]
        sid = int.from_bytes(data[pos + 5:pos + 9], "big") & 0x7fffffff
        hdr_end, end = pos + 8, pos + 9 + ln - 1 if ln else pos + 8  # the last byte of the header, of the frame
        payload = data[pos + 9:pos + 9 + ln]
        if ftype == 4:
            out.append((end, "got_settings_ack" if flags & 1 else "settings", None))
        elif ftype == 6:
            out.append((end, "got_ping_ack" if flags & 1 else "ping", payload))
        elif ftype == 7:
            out.append((end, "got_goaway", (int.from_bytes(payload[:4], "big") & 0x7fffffff, int.from_bytes(payload[4:8], "big"))))
        elif ftype == 0 and sid in grpc and sid not in closed:
            if flags & ~1:
                out.append((hdr_end, "rst", sid))
                closed.add(sid)
            else:
                st = grpc[sid]
                for k, byte in enumerate(payload):
                    if st["dead"]:
                        break
                    if st["left"]:
                        st["left"] -= 1
                    elif st["hdr"] == 0:
                        if byte > 1:
                            out.append((pos + 9 + k, "rst", sid))
                            st["dead"] = True
                        else:
                            st["hdr"], st["len"] = 1, 0
                    else:
                        st["len"] = st["len"] << 8 | byte
                        st["hdr"] += 1
                        if st["hdr"] == 5:
                            st["hdr"], st["left"] = 0, st["len"]
        pos += 9 + ln
    assert pos == len(data)
    return out


def walker_calls(data, streams, bounds):
    """the walker's answer per call ([a, b) byte ranges): (wire, counts, peer record behind the call)"""
    due = walk(data, streams)
    peer = dict(settings_acks=0, ping_acks=0, last_ping_opaque=0, goaways=0, goaway_last_stream=0, goaway_error=0, goaway_call=0)
    res = []
    for n, (a, b) in enumerate(bounds):
        mine = sorted(d for d in due if a <= d[0] < b)
        pings = [ping_ack(v) for _, k, v in mine if k == "ping"]
        queued = [SETTINGS_ACK if k == "settings" else rst_stream(v) for _, k, v in mine if k in ("settings", "rst")]
        for _, k, v in mine:
            if k == "got_settings_ack":
                peer["settings_acks"] += 1
            elif k == "got_ping_ack":
                peer["ping_acks"] += 1
                peer["last_ping_opaque"] = int.from_bytes(v, "little")
            elif k == "got_goaway":
                peer["goaways"] += 1
                peer["goaway_last_stream"], peer["goaway_error"] = v
                peer["goaway_call"] = n + 1
        wire = b"".join(pings + queued)
        counts = (len(pings) + len(queued), -(-len(wire) // 23), len(wire), sum(1 for _, k, _ in mine if k == "settings"),
                  len(pings), sum(1 for _, k, _ in mine if k == "rst"), GOAWAY if any(k == "got_goaway" for _, k, _ in mine) else 0, 0)
        res.append((wire, counts, dict(peer)))
    return res


def random_stream(rng):
    fr = [frame(4, 0, 0, b"".join(rng.randrange(1, 4).to_bytes(2, "big") + rng.randrange(1 << 16).to_bytes(4, "big")
                                  for _ in range(rng.randrange(0, 3))))]  # (a connection begins with SETTINGS)
    for _ in range(rng.randrange(1, 14)):
        kind = rng.randrange(9)
        if kind == 0:
            fr.append(frame(4, 0, 0, b"".join((3).to_bytes(2, "big") + rng.randrange(1 << 16).to_bytes(4, "big")
                                              for _ in range(rng.randrange(0, 3)))))
        elif kind == 1:
            fr.append(frame(4, 1, 0))
        elif kind in (2, 3):
            fr.append(frame(6, kind & 1, 0, bytes(rng.randrange(256) for _ in range(8))))
        elif kind == 4:
            fr.append(frame(7, 0, 0, rng.randrange(1 << 32).to_bytes(4, "big") + rng.randrange(1 << 32).to_bytes(4, "big") +
                            bytes(rng.randrange(256) for _ in range(rng.choice((0, 0, 1, 13, 40))))))
        elif kind == 5:
            fr.append(frame(8, 0, rng.choice((0,) + STREAMS), rng.randrange(1, 1 << 20).to_bytes(4, "big")))
        elif kind == 6:
            fr.append(frame(0, rng.choice((2, 4, 8, 9)), rng.choice(STREAMS), bytes(rng.randrange(0, 12))))  # bad DATA flags
        elif kind == 7:  # a message whose first byte is no gRPC flag, in front of or behind good ones
            good = b"".join(grpc_msg(bytes(rng.randrange(256) for _ in range(rng.randrange(0, 9)))) for _ in range(rng.randrange(0, 3)))
            fr.append(frame(0, 0, rng.choice(STREAMS), good + bytes([rng.randrange(2, 256)]) + bytes(rng.randrange(0, 7))))
        else:
            body = b"".join(grpc_msg(bytes(rng.randrange(256) for _ in range(rng.randrange(0, 20)))) for _ in range(rng.randrange(1, 3)))
            cut = rng.randrange(0, len(body) + 1)  # (a message may span two DATA frames)
            sid = rng.choice(STREAMS)
            fr += [frame(0, 0, sid, body[:cut]), frame(0, 0, sid, body[cut:])]
    return b"".join(fr)


def cut(rng, a, b, k):
    """[a, b) in at most k + 1 non-empty pieces"""
    pts = sorted(set(rng.randrange(a + 1, b) for _ in range(k))) if b - a > 1 else []
    return list(zip([a] + pts, pts + [b]))


def test_model_against_a_byte_at_a_time_walker():
    rng = random.Random(21)
    kinds = set()
    for case in range(2000):
        data = random_stream(rng)
        bounds = cut(rng, 0, len(data), rng.randrange(0, 6))
        want = walker_calls(data, STREAMS, bounds)
        orc = pyorc.H2Parser(False)
        for s in STREAMS:
            assert orc.open_stream(s) == 0
        m = ControlModel()
        for n, (a, b) in enumerate(bounds):
            slices = [data[x:y] for x, y in cut(rng, a, b, rng.choice((0, 1, 3, b - a)))]
            err, ev = oracle_feed(orc, slices)
            assert err == 0, (case, n)
            lens, wire, res = m.reply(ev, slices, err, 1 << 20, 1 << 30)
            assert (wire, res, m.peer) == want[n], (case, n, bounds)
            assert lens == [min(23, len(wire) - o) for o in range(0, len(wire), 23)], (case, n)
            kinds |= {i for i in range(3, 6) if res[i]} | ({"cut"} if m.carry else set())
        assert m.carry is None and m.stats["calls"] == len(bounds)
    assert kinds == {3, 4, 5, "cut"}


def test_the_grpcio_capture_asks_for_one_settings_ack():
    data, _ = grpcio_capture()
    assert data.startswith(PREFACE)
    first = len(PREFACE)
    assert data[first:first + 5] == bytes([0, 0, 36, 4, 0])  # the 36-byte SETTINGS frame leads
    for at in [None] + list(range(first, first + 9 + 36 + 1)):
        orc = pyorc.H2Parser(True)
        m = ControlModel()
        out = []
        for part in ([data] if at is None else [data[:at], data[at:]]):
            err, ev = oracle_feed(orc, [part])
            assert err == 0
            out.append(m.reply(ev, [part], err, 64, 2048))
        lens, wire = sum((o[0] for o in out), []), b"".join(o[1] for o in out)
        assert (lens, wire) == ([9], SETTINGS_ACK), at
        assert sum(o[2][0] for o in out) == 1 and all(o[2][4:] == (0, 0, 0, 0) for o in out), (at, out)
        # the ACK is due in the call that holds the frame's last byte
        assert at is None or (out[0][2][0] == 1) == (at == first + 9 + 36), at
        assert m.peer == dict(settings_acks=1, ping_acks=0, last_ping_opaque=0, goaways=0, goaway_last_stream=0, goaway_error=0,
                              goaway_call=0)
        assert m.stats["settings_acks"] == 1 and m.stats["wire_bytes"] == 9 and m.carry is None


def test_slice_rule():
    # totals of 0, 9, 22, 23, 24, 46 and 47 bytes
    for frames, total, n in (([], 0, 0), ([SETTINGS_ACK], 9, 1), ([SETTINGS_ACK, rst_stream(1)], 22, 1),
                             ([bytes(23)], 23, 1), ([bytes(12), bytes(12)], 24, 2), ([bytes(23), bytes(23)], 46, 2),
                             ([ping_ack(bytes(8)), ping_ack(bytes(8)), rst_stream(3)], 47, 3)):
        lens = cut23(frames)
        assert sum(len(f) for f in frames) == total == sum(lens) and len(lens) == n, (total, lens)
        assert all(x == 23 for x in lens[:-1]) and all(0 < x <= 23 for x in lens)


def test_frame_images():
    assert SETTINGS_ACK == bytes.fromhex("000000040100000000") == frame(4, 1, 0)
    assert ping_ack(bytes(range(1, 9))) == bytes.fromhex("000008060100000000" "0102030405060708") == frame(6, 1, 0, bytes(range(1, 9)))
    assert rst_stream(0x01020305) == bytes.fromhex("0000040300" "01020305" "00000001") == frame(3, 0, 0x01020305, (1).to_bytes(4, "big"))
    # ... and they parse as what they are
    orc = pyorc.H2Parser(False)
    assert orc.open_stream(5) == 0
    err, ev = orc.feed(frame(4, 0, 0) + SETTINGS_ACK + ping_ack(bytes(8)) + rst_stream(5))
    assert err == 0 and [(e[1], e[2], e[3], e[4]) for e in ev if e[0] == pyorc.EV_FRAME] == [(4, 0, 0, 0), (4, 1, 0, 0), (6, 1, 0, 8), (3, 0, 5, 4)]
