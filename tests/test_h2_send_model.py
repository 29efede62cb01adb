"""tests/h2_send_model.py pinned before a device test trusts it: its wire against the oracle's framer under open
windows, the two forms of the grant against each other, windowed calls end to end through the oracle's parser, and its
intake over the capture of a stock gRPC client."""
import random

from oracle import pyorc
from tests.h2_helpers import PREFACE, grpcio_capture
from tests.h2_send_model import (MAXW, SendModel, grant_prefix, grant_sequential, live_of)

LENGTHS = (0, 1, 4, 9, 30, 200, 700)
FRAMES = (1, 2, 5, 6, 7, 14, 23, 100, 16384)


def _table(rng, streams=(1, 3, 5, 7)):
    n = rng.randrange(1, 10)
    return [(bytes(rng.randrange(256) for _ in range(rng.choice(LENGTHS))), rng.choice(streams), rng.randrange(4))
            for _ in range(n)]


def test_open_windows_equal_the_oracles_batch():
    rng = random.Random(11)
    for case in range(300):
        msgs = _table(rng)
        mf = rng.choice(FRAMES)
        m = SendModel(MAXW, MAXW, (1 << 24) - 1)
        live = {s for _, s, _ in msgs}
        lens, wire, res, prog = m.frame(msgs, [0] * len(msgs), mf, 1 << 20, 1 << 30, live)
        wire_o, lens_o = pyorc.h2_frame_batch([b for b, _, _ in msgs], [s for _, s, _ in msgs], [f for _, _, f in msgs], mf)
        assert (wire, lens) == (wire_o, lens_o), (case, mf, [(len(b), s, f) for b, s, f in msgs])
        assert res == (len(msgs), 0, len(lens), res[3], len(wire), sum(5 + len(b) for b, _, _ in msgs), 0, 0)
        assert prog == [5 + len(b) for b, _, _ in msgs]


def test_the_two_forms_of_the_grant_agree():
    rng = random.Random(12)
    for case in range(20000):
        n = rng.randrange(1, 13)
        streams = [rng.choice((1, 3, 5, 7)) for _ in range(n)]
        rem = [rng.randrange(1, 60) for _ in range(n)]
        windows = {s: rng.randrange(-10, 81) for s in (1, 3, 5)}  # (7 is unknown)
        windows[7] = None
        conn = rng.randrange(0, 151)
        a, g = grant_prefix(rem, streams, windows, conn)
        assert g == grant_sequential(rem, streams, windows, conn), (rem, streams, windows, conn)
        assert all(0 <= y <= x <= r for y, x, r in zip(g, a, rem)) and sum(g) <= conn


def test_windowed_calls_round_trip_through_the_oracles_parser():
    rng = random.Random(13)
    for case in range(200):
        msgs = _table(rng, streams=(1, 3, 5))
        msgs = [(b, s, f & 1) for b, s, f in msgs]  # (no END_STREAM: the streams stay for the next case's messages)
        mf = rng.choice((1, 2, 5, 6, 7, 14, 23, 100))
        m = SendModel(rng.randrange(0, 31), rng.randrange(0, 31), 16384)
        live = {1, 3, 5}
        orc = pyorc.H2Parser(False)
        for s in live:
            assert orc.open_stream(s) == 0
        todo, prog, got, calls = list(msgs), [0] * len(msgs), [], 0
        while todo:
            m.conn += rng.randrange(0, 31)
            for s in live:
                m.delta[s] = m.delta.get(s, 0) + rng.randrange(0, 31)
            lens, wire, res, prog = m.frame(todo, prog, mf, 1 << 20, 1 << 30, live)
            assert all(0 < n for n in lens) and sum(lens) == len(wire) == res[4] and res[7] == 0
            rc, ev = orc.feed(wire)
            assert rc == 0
            got.append((wire, ev))
            keep = [i for i, (b, _, _) in enumerate(todo) if prog[i] < 5 + len(b)]
            assert res[0] == len(todo) - len(keep) and res[1] == len(keep)
            todo, prog = [todo[i] for i in keep], [prog[i] for i in keep]
            calls += 1
            assert calls < 10000
        # every stream's messages, in order (MSG_BYTES offsets are offsets into the call's wire)
        back = {}
        partial = {}
        for wire, ev in got:
            for k, a, b, c, d in ev:
                if k == pyorc.EV_MSG_BEGIN:
                    partial[c] = bytearray()
                elif k == pyorc.EV_MSG_BYTES:
                    partial[c] += wire[a:a + b]
                elif k == pyorc.EV_MSG_END:
                    back.setdefault(c, []).append(bytes(partial.pop(c)))
        want = {}
        for b, s, _ in msgs:
            want.setdefault(s, []).append(b)
        assert back == want and not partial, case


def test_inlined_slices_stay_within_23_bytes():
    rng = random.Random(14)
    for case in range(200):
        msgs = _table(rng, streams=(1, 3))
        m = SendModel(rng.randrange(0, 40), rng.randrange(1, 60), 16384)
        mf = rng.choice((1, 5, 6, 23, 100))
        sb_wire = m.frame(msgs, [0] * len(msgs), mf, 1 << 20, 1 << 30, {1, 3})
        lens, wire = sb_wire[0], sb_wire[1]
        # header bytes are inlined: a slice longer than 23 bytes is payload by reference and lies inside a body
        pos = 0
        for n in lens:
            assert n > 0
            if n > 23:
                piece = wire[pos:pos + n]
                assert any(piece in b for b, _, _ in msgs)
            pos += n


def test_intake_over_the_grpcio_capture():
    data, _ = grpcio_capture()
    orc = pyorc.H2Parser(True)
    rc, ev = orc.feed(data)
    assert rc == 0 and data.startswith(PREFACE)
    m = SendModel()
    seen = []
    live = live_of(orc) | {1, 3, 5, 7, 9}  # (judged as if the call's streams were still in the map)
    res = m.intake([e + (0,) for e in ev], [data], 0, live)
    assert res[3] == 1 and (m.iws, m.pmf) == (4194304, 4194304)
    assert res[0] == 7 and res[4] == 0 and res[7] == 0
    assert m.conn == 65535 + 4128769 + 5 and res[1] == 4128769 + 5
    assert {s: m.iws + d for s, d in m.delta.items()} == {s: 4194304 + 5 for s in (1, 3, 5, 7, 9)} and res[2] == 25
    # the frames themselves, read from the wire by the events
    for i, e in enumerate(ev):
        if e[0] == pyorc.EV_FRAME and e[1] == 8:
            p = ev[i + 1]
            assert p[0] == pyorc.EV_PAYLOAD and p[2] == 4 and p[3] == 1
            seen.append((e[3], int.from_bytes(data[p[1]:p[1] + 4], "big")))
    assert seen[0] == (0, 4128769) and sorted(seen[1:]) == [(0, 5), (1, 5), (3, 5), (5, 5), (7, 5), (9, 5)]
    # with the map as the oracle has it behind the call, only the streams still there keep an entry
    m2 = SendModel()
    m2.intake([e + (0,) for e in ev], [data], 0, live_of(orc))
    assert set(m2.delta) == live_of(orc) & {1, 3, 5, 7, 9} and m2.conn == m.conn
