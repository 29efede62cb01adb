"""Header blocks on many links: the decoders of a table of transports in the same six launches (k_h2_links_hpack_*,
grdma_h2_hpack_decode_batch, h2dev.decode_batch).  Every item of a batch is compared exactly with its own link's
HpackModel (tests/h2_hpack_model.py) through decode_batch of tests/h2_links_hpack_lib.py: result block, the three targets
whole, the dynamic table and the counters.  The blocks are small: the point is the link indexing, not the decoder's
edges (tests/test_zz_gpu_h2_hpack.py, tests/test_zz_gpu_h2_hpack_sweep.py)."""
import json
import os
import random

import pytest

from tests.h2_control_lib import cut_at, data, ping, settings
from tests.h2_device_lib import same
from tests.h2_helpers import grpcio_capture
from tests.h2_hpack_lib import Targets, headers_frames, indexed, literal, own_sequence, size_update
from tests.h2_hpack_model import ERR_INDEX, FAILED, LOST, OPEN
from tests.h2_links_hpack_lib import HH, decode_batch, decode_batch_raw

pytestmark = pytest.mark.gpu

NINE = bytes.fromhex("c4c38386c2c1c0bfbe")  # the capture's fully indexed block
INVALID = -2  # -GRDMA_ERR_INVALID


def word(flags, err=0, stream=0):
    return flags | err << 8 | stream << 32


def _deflated():
    """a sequence of blocks from nghttp2's deflater as tests/golden/h2_hpack_vectors.json keeps it"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "h2_hpack_vectors.json")
    return [bytes.fromhex(b["hex"]) for b in json.load(open(path))["deflated"][0]]


def _close(hs):
    for h in hs:
        h.close()


def test_nine_links_in_shuffled_order_over_three_calls(gpu):
    capture, _ = grpcio_capture()
    deflated, own = _deflated(), [b for b, _ in own_sequence(11, 3)]
    assert len(deflated) == 3 and any(b[0] & 0xe0 == 0x20 for b in own)  # (a size update leads one of them)
    cut = headers_frames(7, literal(b"name-one", b"value-one") + literal(b"name-two", b"v" * 40, hv=True) + indexed(62) + indexed(63),
                         cont=(5, 20, 41))
    at = 9 + 5 + 9 + 15 + 9 + 10  # ten bytes into the second CONTINUATION
    ones = headers_frames(1, literal(b"a", b"b" * 10) + indexed(62)) + ping(3)
    fill = b"".join(literal(b"key%d" % k, b"val%d" % k) for k in range(8))  # 40 bytes each into 256: two go
    hs = [HH(gpu, prefix=True), HH(gpu), HH(gpu), HH(gpu, streams=(1, 3)), HH(gpu), HH(gpu), HH(gpu), HH(gpu, setting=256), HH(gpu)]
    rounds = (
        [[capture[:333]], [headers_frames(1, deflated[0])], [headers_frames(1, own[0])], [data(1) + data(3, b"x" * 50)], [],
         [ones[i:i + 1] for i in range(len(ones))],
         [headers_frames(1, NINE[2:4] + literal(b"a", b"b"), flags=1, pad=3, priority=True, cont=(1,))],
         [headers_frames(1, fill)], [cut[:at]]],
        [[capture[333:529]], cut_at(headers_frames(3, deflated[1], cont=(100,)), 50), [ping(1) + headers_frames(3, own[1])], [data(3)], [],
         [bytes([b]) for b in headers_frames(3, indexed(62))], [headers_frames(3, indexed(62), pad=0, priority=True)],
         [headers_frames(3, indexed(62) + indexed(67) + literal(62, b"new"))], [cut[at:]]],
        [[capture[529:]], [headers_frames(5, deflated[2])], [headers_frames(5, own[2]) + settings(1)], [data(1, b"y" * 20)], [], [],
         [headers_frames(5, literal(62, b"c"), pad=5)], [headers_frames(5, indexed(63) + indexed(62) + indexed(66))],
         [headers_frames(9, indexed(62) + indexed(63))]])
    rng = random.Random(7)
    for n, calls in enumerate(rounds):
        for h, slices in zip(hs, calls):
            h.deframe(slices)
        order = list(range(9))
        rng.shuffle(order)
        out = decode_batch(hs, order)
        assert all(out[i][1][6:] == (OPEN if (n, i) in ((0, 0), (0, 8)) else 0, 0) for i in range(9)), n
        assert out[3][1] == out[4][1] == (0, 0, 0, 0, 0, 0, 0, 0)  # only DATA; nothing at all
        if n == 0:
            assert out[0][1][0] == 0 and out[8][0] == [] and out[7][1][3:6] == (8, 2, 240)  # cut blocks; the table evicts
        elif n == 1:
            assert [s for s, _, _ in out[0][0]] == [1, 3, 5] and out[8][1][:2] == (1, 4)  # (the carry of batch call 1)
            assert [f[0] for f in out[8][0][0][2]] == [b"name-one", b"name-two", b"name-two", b"name-one"]
            assert [f[:2] for f in out[7][0][0][2]] == [(b"key7", b"val7"), (b"key2", b"val2"), (b"key7", b"new")]
        else:
            assert [s for s, _, _ in out[0][0]] == [7, 9]
            # entries of batch call 1 and of batch call 2, referenced in call 3
            assert [f[:2] for f in out[7][0][0][2]] == [(b"key7", b"val7"), (b"key7", b"new"), (b"key4", b"val4")]
            assert [f[:2] for f in out[6][0][0][2]] == [(b"a", b"c")] and out[5][1][0] == 0
    _close(hs)


def test_batch_against_single_on_twin_parsers(gpu):
    a, b, c = (HH(gpu, setting=200) for _ in range(3))
    wire = headers_frames(5, literal(62, b"w" * 30) + indexed(63) + literal(b"third", b"3", mode=2), cont=(7,))
    for slices in ([headers_frames(1, literal(b"alpha", b"1") + indexed(62)) + headers_frames(3, literal(62, b"2") + indexed(63))],
                   [ping(2) + wire[:25]], [wire[25:] + headers_frames(7, size_update(100) + indexed(62))]):
        for h in (a, b, c):
            h.deframe(slices)
        single = a.decode()
        out = decode_batch([b, c], [1, 0])
        assert out[0] == out[1] == single
        same(a.target.read(), b.target.read(), "twin targets")
        same(b.target.read(), c.target.read(), "twin targets")
        stats = [{k: v for k, v in h.dec.stats().items() if k != "kernel_us"} for h in (a, b, c)]
        same((b.dec.table(), stats[1]), (a.dec.table(), stats[0]), "twin tables and counters")
        same((c.dec.table(), stats[2]), (a.dec.table(), stats[0]), "twin tables and counters")
    _close((a, b, c))


def test_trouble_stays_with_its_link(gpu):
    hs = [HH(gpu) for _ in range(5)]
    for h in hs:
        h.deframe([headers_frames(1, literal(b"a", b"1"))])
    decode_batch(hs, [4, 2, 0, 3, 1])
    # link 0: an HPACK error in the second block of three; link 1: its event list overflows; link 2: a fields cap one too
    # small; 3 and 4 are exact
    good = headers_frames(3, indexed(62) + literal(b"b", b"2")) + headers_frames(5, indexed(62) + indexed(63) + literal(b"c", b"3"))
    hs[0].deframe([headers_frames(3, literal(b"n", b"v")) + headers_frames(5, indexed(62) + indexed(64)) + headers_frames(7, b"\x82")])
    with pytest.raises(gpu.GrdmaError, match="error 5"):
        hs[1].deframe([headers_frames(3, b"\x82") * 8], ev_cap=4, checked=False)
    for i in (2, 3, 4):
        hs[i].deframe([good])
    before = (list(hs[2].model.table.entries), dict(hs[2].model.stats))
    out = decode_batch(hs, [2, 1, 0, 3, 4], caps={2: (2, 4, 64)}, lost=(1,))  # (the library: three items without overflow)
    assert out[0][1] == (1, 1, 2, 1, 0, 68, word(FAILED, ERR_INDEX, 5), 0) and out[0][0][0][2] == [(b"n", b"v", 1)]
    assert out[1][1] == (0, 0, 0, 0, 0, 34, LOST, 2)
    assert out[2][1][:3] == (2, 5, 10) and out[2][1][7] == 1 and (list(hs[2].model.table.entries), hs[2].model.stats) == before
    assert out[3] == out[4] and out[3][1] == (2, 5, 10, 2, 0, 34 * 3, 0, 0)
    # the overflowed item is not taken: beside a link whose call is, the batch is refused with nothing run
    rc, _ = decode_batch_raw(hs, [2, 0])
    assert rc == INVALID
    same(hs[2].target.read(), tuple(bytes([0xA5]) * len(x) for x in hs[2].target.read()), "a refused batch writes nothing")
    assert hs[2].decode() == out[3]  # repeated alone, with room
    # ... and inside a later batch; the failed link stays failed, the lost one lost
    hs[0].deframe([headers_frames(9, b"\x82")])
    hs[1].deframe([headers_frames(5, b"\x82")], checked=False)  # (the parser lost its place in the overflowing call)
    for i in (2, 3, 4):
        hs[i].deframe([headers_frames(7, indexed(62) + indexed(64))])
    out = decode_batch(hs, [3, 2, 0, 1], caps={2: (1, 2, 3)})
    assert out[0][1] == (0, 0, 0, 0, 0, 68, word(FAILED, ERR_INDEX, 5), 0) and out[1][1] == (0, 0, 0, 0, 0, 34, LOST, 0)
    assert out[2][1] == (1, 2, 4, 0, 0, 34 * 3, 0, 1) and out[3][1] == (1, 2, 4, 0, 0, 34 * 3, 0, 0)
    later = decode_batch(hs, [4, 2])
    assert later[2] == later[4] == out[3]
    # the return value counts the items without overflow
    for i in (2, 3, 4):
        hs[i].deframe([headers_frames(9, indexed(63))])
    rc, res = decode_batch_raw(hs, [2, 3, 4], caps={3: (4, 4, 1)})
    assert rc == 2 and [r[7] for r in res] == [0, 1, 0] and res[1][:3] == (1, 1, 2)
    _close(hs)


@pytest.mark.parametrize("nlinks", [33, 256])
def test_many_links_each_against_its_own_table(gpu, nlinks):
    # (33: one more than a power of two and more than the emulator's grid; 256: GRDMA_H2_BATCH_MAX)
    hs = [HH(gpu, setting=100 + 10 * (i % 9), caps=(4, 16, 256)) for i in range(nlinks)]
    for i, h in enumerate(hs):
        name = b"k%03d" % i
        wire = headers_frames(1, literal(name, b"v" * (i % 5)) + literal(b"second", b"x" * 20)) + headers_frames(3, indexed(63) + indexed(62))
        if i % 2:  # (an insertion by name reference: the smaller tables evict)
            wire += headers_frames(5, literal(63, b"i%d" % i) + indexed(62))
        h.deframe([wire])
    order = list(range(nlinks))
    random.Random(8).shuffle(order)
    out = decode_batch(hs, order)
    for i in range(nlinks):
        name = b"k%03d" % i
        assert out[i][1][:2] == ((3, 6) if i % 2 else (2, 4)) and out[i][1][6:] == (0, 0), i
        assert [f[:2] for f in out[i][0][1][2]] == [(name, b"v" * (i % 5)), (b"second", b"x" * 20)], i
        if i % 2:
            assert [f[:2] for f in out[i][0][2][2]] == [(name, b"i%d" % i)] * 2 and hs[i].model.table.entries[0] == (name, b"i%d" % i), i
    assert {h.model.table.max_size for h in hs} == {100 + 10 * k for k in range(9)} and any(o[1][4] for o in out.values())
    _close(hs)


def test_uneven_links(gpu):
    # a scratch size taken from the wrong link overruns or truncates: about 60 KB of block beside two bytes and nothing
    big = b"".join(literal(b"x-%03d" % k, bytes([97 + k % 26]) * 190, mode=1 if k % 50 == 0 else 2) for k in range(300))
    assert 59000 < len(big) < 61000
    hs = [HH(gpu, max_block=1 << 17, caps=(4, 512, 1 << 17)), HH(gpu, caps=(4, 16, 256)), HH(gpu, caps=(4, 64, 1 << 13))]
    hs[0].deframe([headers_frames(1, big, cont=(16000, 32000, 48000))])
    hs[1].deframe([headers_frames(1, b"\x82\x86")])
    hs[2].deframe([])
    out = decode_batch(hs, [1, 0, 2])
    assert out[0][1][:3] == (1, 300, 300 * 195) and out[0][1][6:] == (0, 0) and out[1][1] == (1, 2, 21, 0, 0, 0, 0, 0) and out[2][1][:3] == (0, 0, 0)
    # ... and the other way round in the next call: the small link's scratch has not grown with the large one's
    hs[0].deframe([headers_frames(3, b"\x82")])
    hs[1].deframe([])
    hs[2].deframe([headers_frames(1, big[:199 * 40], cont=(5000,))])
    out = decode_batch(hs, [2, 1, 0])
    assert out[2][1][:3] == (1, 40, 40 * 195) and out[2][1][6:] == (0, 0) and out[0][1][:2] == (1, 1)
    _close(hs)


def test_refusals(gpu):
    import ctypes as C
    from grpc_rdma_amd import h2dev
    hs = [HH(gpu, caps=(4, 16, 256)) for _ in range(2)]
    fresh, taken, gone = (HH(gpu, caps=(4, 16, 256)) for _ in range(3))
    for h in (taken, gone):
        h.feed([headers_frames(1, b"\x82")])
    gone.deframe([headers_frames(3, b"\x82")])
    gone.parser.close()
    spare = Targets(gpu, 4, 16, 256)

    def item(h, t=None):
        return (h.dec,) + (t or h.target).args()

    def bad_target(k, v):
        a = list(spare.args())
        a[k] = v(a[k])
        return (hs[1].dec,) + tuple(a)

    cases = [("none", lambda: [], "BATCH_MAX"), ("257 items", lambda: [item(hs[0])] * 257, "BATCH_MAX"),
             ("no decoder", lambda: [item(hs[0]), (None,) + spare.args()], "without decoder"),
             ("twice", lambda: [item(hs[0]), item(hs[1]), item(hs[0], spare)], "twice"),
             ("parser gone", lambda: [item(hs[0]), item(gone, spare)], "parser is gone"),
             ("nothing deframed", lambda: [item(hs[0]), item(fresh, spare)], "deframed nothing"),
             ("taken", lambda: [item(hs[0]), item(taken, spare)], "taken in already")]
    cases += [("target %d zero" % k, lambda k=k: [item(hs[0]), bad_target(k, lambda x: 0)], "null, zero or misaligned") for k in range(6)]
    cases += [("target %d misaligned" % k, lambda k=k: [item(hs[0]), bad_target(k, lambda x: x + 8)], "null, zero or misaligned") for k in (0, 2, 4)]
    cases += [("no item array", None, None), ("no result array", None, None)]
    for n, (what, items, why) in enumerate(cases):
        for h in hs:
            h.deframe([headers_frames(2 * n + 1, (literal(b"n%d" % n, b"v") if n % 3 == 0 else b"") + indexed(62 if n else 2))])
            h.target = Targets(gpu, *h.caps)
        if items is None:
            arr, out = (h2dev.H2HpackItem * 1)(), (C.c_uint64 * 8)()
            arr[0].hpack = hs[0].dec.h
            (arr[0].d_blocks, arr[0].blocks_cap, arr[0].d_fields, arr[0].fields_cap, arr[0].d_strings, arr[0].strings_cap) = hs[0].target.args()
            rc = h2dev.load().grdma_h2_hpack_decode_batch(*((None, 1, out) if what == "no item array" else (arr, 1, None)))
            same(rc, INVALID, what)
        else:
            with pytest.raises(gpu.GrdmaError, match=why):
                h2dev.decode_batch(items())
        for t in (hs[0].target, hs[1].target, spare):
            same(t.read(), tuple(bytes([0xA5]) * len(x) for x in t.read()), what + ": nothing written")
        out = decode_batch(hs, [1, 0])  # (nothing ran, nothing changed: both calls are still to be taken, and match)
        assert out[0] == out[1] and out[0][1][0] == 1 and out[0][1][6:] == (0, 0), what
    assert taken.dec.stats()["calls"] == 1 and fresh.dec.stats()["calls"] == 0 and gone.dec.stats()["calls"] == 1
    gone.dec.close()
    _close(hs + [fresh, taken])


@pytest.mark.parametrize("first", ["decoders", "others"])
def test_the_other_followers_on_the_same_deframings(gpu, first):
    from grpc_rdma_amd import h2dev
    from tests.h2_control_lib import Target, bad_flags
    from tests.h2_control_model import ControlModel
    from tests.h2_send_model import SendModel, live_of
    hs = [HH(gpu, streams=(1, 3)) for _ in range(3)]
    ctls, cms = [h2dev.ControlReplies(h.parser) for h in hs], [ControlModel() for _ in hs]
    sws, sms = [h2dev.SendWindows(h.parser) for h in hs], [SendModel() for _ in hs]
    hd = headers_frames(1, literal(b"k", b"v" * 30) + indexed(62))
    calls = ([settings(1) + ping(5) + hd[:20]], [hd[20:] + data(3, b"y" * 50) + bad_flags(3) + ping(6) + headers_frames(3, indexed(62))])
    for n, slices in enumerate(calls):
        for i, h in enumerate(hs):
            h.deframe(slices if i != 2 else ([ping(7)] + slices, slices + [ping(8)])[n])  # (link 2: slices and PINGs of its own)

        def others():
            ts = [Target(gpu, 8) for _ in hs]
            exp = [cm.reply(h.last[1], h.last_slices, h.last[0], 8, 256) for h, cm in zip(hs, cms)]
            got = h2dev.control_batch([(ctl, t.slices.ptr, 8, t.hdr.ptr, 256) for ctl, t in zip(ctls, ts)][::-1])[::-1]
            for i, (t, (lens, wire, res), (sl, r)) in enumerate(zip(ts, exp, got)):
                same(r, res, "writer %d: result" % i)
                t.check(gpu, sl, lens, wire, "writer %d" % i)
            same(h2dev.intake_batch(sws), [sm.intake(h.last[1], h.last_slices, h.last[0], live_of(h.pp.orc)) for h, sm in zip(hs, sms)],
                 "intake: results")

        for step in ((lambda: decode_batch(hs, [2, 0, 1]), others) if first == "decoders" else (others, lambda: decode_batch(hs, [2, 0, 1]))):
            step()
    assert all(h.model.stats["blocks"] == 2 and h.model.stats["fields"] == 3 for h in hs) and cms[2].stats["ping_acks"] == 4
    for x in ctls + sws:
        x.close()
    _close(hs)
