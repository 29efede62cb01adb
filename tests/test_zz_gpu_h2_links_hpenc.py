"""Header blocks, sending, on many links: the encoders of a table of connections in the same four launches
(k_h2_links_hpenc_*, grdma_h2_hpenc_encode_batch, h2dev.encode_batch).  Every item of a batch is compared exactly with
its own link's HpencModel (tests/h2_hpenc_model.py) through encode_batch of tests/h2_links_hpenc_lib.py: the result
tuple, the wire arena and the block-wire table whole, the dynamic table and the counters.  The lists are small: the point
is the link indexing, the per-item outcomes and the second run, not the encoder's edges (tests/test_zz_gpu_h2_hpenc.py)."""
import copy
import random

import pytest

from tests.h2_device_lib import same
from tests.h2_hpenc_lib import ERR2, Wire, fill
from tests.h2_hpenc_model import BAD_INPUT, ERR_STREAM, ERR_STRING, HpencModel, deframe, enc_int, pack
from tests.h2_links_hpenc_lib import HE, Input, compare, encode_batch, prepare, table_words, unchanged

pytestmark = pytest.mark.gpu

RAW = b"\x01"  # a byte whose code has 23 bits: strings of it go raw
INVALID = -2   # -GRDMA_ERR_INVALID
BIG = 1 << 40


def _close(hs):
    for h in hs:
        h.close()


def _calls(h):
    return h.enc.stats()["calls"]


def test_nine_links_in_shuffled_order_over_three_calls(gpu):
    hs = [HE(gpu, 200 if i == 4 else 4096) for i in range(9)]  # (link 4: room for four of its entries)
    rng = random.Random(7)

    def own(i, n):
        """link i's lists of call n: headers of its own fields under the hints 0 to 3, then trailers"""
        fs = [(nm, v, (i + k) % 4) for k, (nm, v) in enumerate(fill(4 + i, b"l%d" % i))]
        if n == 2:  # the older half again, and new ones
            fs = fs[:2 + i // 2] + [(nm, v, (i + k) % 4) for k, (nm, v) in enumerate(fill(2, b"m%d" % i))]
        return [(2 * n + 1, 0, fs),
                (2 * n + 1, 1, [(b"grpc-status", b"%d" % (i % 3), 1), (b"grpc-message", b"link %d" % i if n < 2 else b"call %d" % n, i % 4)])]

    first = {}
    for n in range(3):
        order = list(range(9))
        rng.shuffle(order)
        count, out = encode_batch(hs, order, lists={i: own(i, n) for i in range(9)})
        assert count == 9 and all(out[i][2][:2] == (2, 2) and out[i][2][6:] == (0, 0) for i in range(9)), n
        if n == 0:
            first = out
            assert all(out[i][2][3] >= 2 for i in range(9)) and out[4][2][4] > 0  # every link inserts; link 4 evicts
        elif n == 1:
            # the same lists against the entries call 1 inserted on that link: nothing new where nothing was evicted,
            # and the indexed forms are shorter
            assert all(out[i][2][3] == 0 and out[i][2][2] < first[i][2][2] for i in range(9) if i != 4)
            assert out[4][2][3] > 0 and out[4][2][4] > 0
            # grpc-status is the newest entry but one where grpc-message was inserted behind it, else the newest
            assert all(deframe(out[i][0])[1][2][0] == (0xbf if i % 4 < 2 else 0xbe) for i in range(9) if i != 4)
        else:
            assert all((out[i][2][3] >= 1) == (i % 4 != 2) for i in range(9))  # (hints 2 and 3 alone insert nothing)
    _close(hs)


def test_batch_against_single_on_twin_encoders(gpu):
    a, b, c = (HE(gpu, 300) for _ in range(3))
    rounds = ([(1, 0, fill(5)), (3, 1, [(b"grpc-status", b"0", 1)])],
              [(5, 0, fill(7)[3:]), (5, 1, [(b"grpc-status", b"0", 1), (b"grpc-message", b"", 2)])],
              [(7, 1, fill(3) + [(b":status", b"200", 1)])])
    for n, lists in enumerate(rounds):
        if n == 1:
            for h in (a, b, c):
                h.set_peer(50)
                h.set_peer(200)  # lowered, then raised: two size updates lead the block
        single = a.encode(lists)
        count, out = encode_batch([b, c], [1, 0], lists={0: lists, 1: lists})
        assert count == 2 and out[0] == out[1] == single
        same(b.out.wire.read(), c.out.wire.read(), "twin wire arenas")
        same(b.out.bw.read(), c.out.bw.read(), "twin block-wire tables")
        same(b.out.wire.read()[:len(single[0])], single[0], "the batch's wire against the single call's")
        stats = [{k: v for k, v in h.enc.stats().items() if k != "kernel_us"} for h in (a, b, c)]
        same((b.enc.table(), stats[1]), (a.enc.table(), stats[0]), "twin tables and counters")
        same((c.enc.table(), stats[2]), (a.enc.table(), stats[0]), "twin tables and counters")
    _close((a, b, c))


def test_trouble_stays_with_its_link(gpu):
    hs = [HE(gpu) for _ in range(7)]
    for i in (2, 3):
        hs[i].set_peer(300)  # (pending: a refused call leaves it pending)
    two = [(1, 0, fill(2, b"a")), (3, 0, fill(2, b"b"))]
    blocks, fields, arena = pack(two)
    bad_stream = ([blocks[0], (0, 2, 2, 0)], fields, arena)
    no, vo, nl, vl = fields[1]
    bad_string = (blocks, [fields[0], (no, len(arena) - 1, nl, 4)] + fields[2:], arena)
    l2, l3 = [(1, 0, fill(5)), (3, 1, fill(8))], [(1, 0, fill(3)), (3, 0, fill(4)), (5, 1, fill(2))]
    need2 = copy.deepcopy(hs[2].model).encode(*pack(l2), BIG, BIG)[2]
    shared = ([(1, 0, 40, 0), (3, 0, 40, 0), (5, 0, 40, 1)], pack([(1, 0, fill(40))])[1], pack([(1, 0, fill(40))])[2])
    good = [(1, 0, fill(3) + [(b":status", b"200", 1)]), (1, 1, [(b"grpc-status", b"0", 1)])]
    count, out = encode_batch(hs, [5, 2, 0, 4, 3, 1, 6], raw={0: bad_stream, 1: bad_string, 4: shared},
                              lists={2: l2, 3: l3, 5: good, 6: good}, caps={2: (need2[2] - 1, None), 3: (None, 2)})
    assert count == 3  # exactly the items on the wire: 4, 5 and 6
    assert out[0][2] == (0, 0, 0, 0, 0, 0, BAD_INPUT | ERR_STREAM << 8 | 1 << 32, 0)
    assert out[1][2] == (0, 0, 0, 0, 0, 0, BAD_INPUT | ERR_STRING << 8 | 0 << 32, 0)
    assert out[2][2] == need2[:7] + (1,) and out[3][2][:2] == (3, 3) and out[3][2][7] == 1
    assert out[4][2][:2] == (3, 3) and out[4][2][3] == 40 and out[4][2][6:] == (0, 0)  # 120 occurrences over 40 fields: the second run
    assert out[5] == out[6] and out[5][2][:2] == (2, 2)
    # nobody was committed twice, and the refused ones not at all
    assert [_calls(h) for h in hs] == [0, 0, 0, 0, 1, 1, 1]
    # the two cap items again, with room: alone, and inside a later batch -- what a never-refused model gives
    refs = [HpencModel(), HpencModel()]
    want = []
    for ref, lists in zip(refs, (l2, l3)):
        ref.set_peer(300, 16384)
        want.append(ref.encode(*pack(lists), BIG, BIG)[:3])
    assert hs[2].encode(l2) == want[0]
    count, later = encode_batch(hs, [6, 3, 5], lists={3: l3, 5: good, 6: good})
    assert count == 3 and later[3] == want[1] and deframe(later[3][0])[0][2].startswith(enc_int(300, 5, 0x20))
    assert [_calls(h) for h in hs] == [0, 0, 1, 1, 1, 2, 2]
    _close(hs)


def test_per_link_peer_settings_in_one_call(gpu):
    hs = [HE(gpu, 0), HE(gpu, 8192), HE(gpu), HE(gpu, 4096, 32768), HE(gpu, 4096, 16384)]
    small = {i: [(1, 0, fill(3, b"p%d" % i))] for i in range(5)}
    count, out = encode_batch(hs, [3, 1, 4, 0, 2], lists=small)
    assert count == 5
    assert out[0][2][3] == 0 and not hs[0].model.table.entries                  # size 0: nothing is ever inserted
    assert deframe(out[1][0])[0][2].startswith(enc_int(8192, 5, 0x20) + b"\x40")  # created above 4096: one update leads
    assert out[2][2][3] == 3 and deframe(out[2][0])[0][2][0] == 0x40
    hs[2].set_peer(50)
    hs[2].set_peer(200)  # lowered, then raised
    big = [(5, 1, [(b"x-f", RAW * 16500, 2)]), (7, 0, fill(3, b"q"))]
    count, out = encode_batch(hs, [0, 4, 2, 3, 1], lists={0: small[0], 1: small[1], 2: small[2], 3: big, 4: big})
    assert count == 5
    assert deframe(out[2][0])[0][2].startswith(enc_int(50, 5, 0x20) + enc_int(200, 5, 0x20)) and out[2][2][4] == 2  # (50 bytes keep the newest entry)
    assert deframe(out[1][0])[0][2] == b"\xc0\xbf\xbe"
    # the same block of more than 16384 bytes: one frame at 32768, a CONTINUATION and a field cut by the frame at 16384
    assert out[3][2][:2] == (2, 2) and out[4][2][:2] == (2, 3) and out[4][2][2] == out[3][2][2] + 9
    assert out[3][0][3] == 1 and out[3][0][4] == 0x05 and out[4][0][4] == 0x01
    assert out[4][0][9 + 16384 + 3:9 + 16384 + 5] == b"\x09\x04" and out[4][0][9 + 16383] == out[4][0][18 + 16384] == RAW[0]
    assert out[3][1][0][2] == 1 and out[4][1][0][2] == 2
    _close(hs)


def test_uneven_links(gpu):
    # a scratch size, a block count or an occurrence count taken from the wrong link overruns or truncates
    hs = [HE(gpu) for _ in range(6)]
    hs[4].set_peer(100)
    walk = [(nm, v, 1 if k % 50 == 0 else 2) for k, (nm, v) in enumerate(fill(600))]  # three steps of the walk, 12 insertions
    lists = {0: [(1, 0, [(b":method", b"GET", 1)])], 1: [(3, 1, [(b"x-one", b"1", 1)])], 2: [(1, 0, []), (3, 1, []), (5, 0, [])],
             3: [(1, 0, walk)], 4: [], 5: [(2 * k + 1, k & 1, [(b"x-k", b"%d" % (k % 7), 1)]) for k in range(300)]}
    count, out = encode_batch(hs, [3, 0, 4, 2, 5, 1], lists=lists)
    assert count == 6  # (the link without blocks counts: its call succeeded, as the single call says)
    assert out[0][2][:3] == (1, 1, 10) and out[1][2][:2] == (1, 1) and out[2][2][:3] == (3, 3, 27)
    assert out[3][2][:2] == (1, 1) and out[3][2][3] == 12 and out[4][2] == (0, 0, 0, 0, 0, 0, 0, 0)
    assert out[5][2][:2] == (300, 300) and out[5][2][3] == 7
    # ... and the other way round: no link's tables have grown with another's; the link without blocks committed no peer
    # settings, its size update leads its first block now
    lists = {0: [(1, 0, walk[:300])], 1: [], 2: [(1, 0, [(b"x-one", b"1", 1)])], 3: [(1, 0, [])], 4: [(1, 0, [(b"x-one", b"1", 1)])],
             5: [(1, 0, [(b"x-k", b"3", 1)])]}
    count, out = encode_batch(hs, [1, 5, 0, 2, 4, 3], lists=lists)
    assert count == 6 and out[0][2][3] == 6 and out[3][2][:3] == (1, 1, 9) and out[5][0][9:] == b"\xc1"
    assert deframe(out[4][0])[0][2].startswith(enc_int(100, 5, 0x20) + b"\x40") and hs[4].model.table.max_size == 100
    _close(hs)


@pytest.mark.parametrize("nlinks", [33, 256])
def test_many_links_each_against_its_own_table(gpu, nlinks):
    # (33: one more than a power of two and more than the emulator's grid; 256: GRDMA_H2_BATCH_MAX)
    hs = [HE(gpu, 100 + 10 * (i % 9)) for i in range(nlinks)]

    def key(i):
        return (b"k%03d" % i, b"v" * (i % 5), 1)

    lists = {i: [(1, 0, [key(i), (b"second", b"x" * 20, i % 4), (b":status", b"200", 1)]), (3, 1, [key(i), (b"grpc-status", b"%d" % (i % 3), 1)])]
             for i in range(nlinks)}
    order = list(range(nlinks))
    random.Random(8).shuffle(order)
    count, out = encode_batch(hs, order, lists=lists)
    assert count == nlinks
    for i in range(nlinks):
        assert out[i][2][:2] == (2, 2) and out[i][2][6:] == (0, 0) and deframe(out[i][0])[1][2][0] in (0xbe, 0xbf), i
    # the second call references what the first one inserted on that link
    lists = {i: [(5, 0, [(b"grpc-status", b"%d" % (i % 3), 1), key(i)]), (5, 1, [(key(i)[0], b"new", 1), (key(i)[0], b"new", 1)])]
             for i in range(nlinks)}
    random.Random(9).shuffle(order)
    count, out = encode_batch(hs, order, lists=lists)
    assert count == nlinks
    for i in range(nlinks):
        first, second = [b for _, _, b in deframe(out[i][0])]
        # (the small tables that took `second` in have evicted the key: there it is a literal again)
        assert first[0] == 0xbe and (first[1] & 0x80 or first[1] == 0x40) and second[0] & 0xc0 == 0x40 and second[0] & 0x3f >= 62 and second[-1] == 0xbe, i
        assert out[i][2][3] == (1 if first[1] & 0x80 else 2) and hs[i].model.table.entries[0] == (key(i)[0], b"new"), i
    assert {h.model.table.max_size for h in hs} == {100 + 10 * k for k in range(9)} and any(o[2][4] for o in out.values())
    _close(hs)


def test_one_input_for_many_links(gpu):
    # a proxy fans one header list out: eight encoders in different table states read the SAME three device tables
    hs = [HE(gpu, (0, 100, 200, 4096)[i % 4], 16384 if i < 4 else 20000) for i in range(8)]
    count, _ = encode_batch(hs, [1, 3, 5, 7], lists={i: [(1, 0, fill(i))] for i in (1, 3, 5, 7)})  # (some know some of the fields)
    assert count == 4
    hs[6].set_peer(64)
    lists = [(9, 0, fill(6) + [(b":status", b"200", 1), (b"x-secret", b"s" * 30, 3)]), (9, 1, [(b"grpc-status", b"0", 1), fill(6)[5]])]
    tables = pack(lists)
    inp = Input(gpu, *tables)
    order = [6, 0, 3, 7, 1, 5, 2, 4]
    count, out = encode_batch(hs, order, device={i: (inp.args(), tables) for i in order})
    assert count == 8 and len({out[i][0] for i in order}) >= 5  # one input, many wires
    assert out[7][2][3] == 1 and out[0][2][3] == 0 and out[6][0][9:11] == enc_int(64, 5, 0x20)
    same(inp.fields.read()[:16 * len(tables[1])], b"".join(int(w).to_bytes(4, "little") for r in tables[1] for w in r), "the shared input stands")
    _close(hs)


def test_decoder_output_forwarded_on_three_links(gpu):
    from grpc_rdma_amd import h2dev
    from tests.h2_hpack_lib import HH, headers_frames, indexed, literal
    from tests.h2_hpack_model import HpackModel
    from tests.h2_links_hpack_lib import _step
    hhs, hes = [HH(gpu, caps=(8, 32, 512)) for _ in range(3)], [HE(gpu) for _ in range(3)]
    wires = [headers_frames(1, b"\x82\x86" + literal(b"x-a", b"1") + indexed(62)) + headers_frames(3, indexed(62) + literal(b"x-b", b"2", mode=2), flags=1),
             headers_frames(5, literal(b"grpc-status", b"0") + literal(62, b"1", mode=3)),
             headers_frames(7, literal(b"k", b"v" * 40, hv=True) + indexed(62) + indexed(62), cont=(10,)) + headers_frames(9, b"\x88", flags=1)]
    order = [2, 0, 1]
    for h, w in zip(hhs, wires):
        h.deframe([w])
    decoded = _step(hhs, order, None, ())  # (the decoders' models: what the targets will hold, and how much of it)
    device = {}
    for i in order:
        blocks, fields, strings, _res = decoded[i]
        t = hhs[i].target
        device[i] = ((t.blocks.ptr, len(blocks), t.fields.ptr, len(fields), t.strings.ptr, len(strings)), (blocks, fields, strings))
    items, exp = prepare(hes, order, device=device)
    # the decoders' three device targets, unchanged, are the encoders' input: no host step between the two calls
    _, dgot = h2dev.decode_batch([(hhs[i].dec,) + hhs[i].target.args() for i in order])
    count, got = h2dev.encode_batch(items)
    out = compare(hes, order, exp, count, got)
    assert count == 3
    for k, i in enumerate(order):
        blocks, fields, strings, res = decoded[i]
        same(dgot[k], res, "decoder %d: result" % i)
        same(table_words(hhs[i].target.blocks.read(), len(blocks)), [tuple(b) for b in blocks], "decoder %d: the block table" % i)
        hhs[i].check()
        sent = [(stream, flags & 1, [(strings[no:no + (nl & 0xffffff)], strings[vo:vo + vl], nl >> 24) for no, vo, nl, vl in fields[first:first + n]])
                for stream, first, n, flags in blocks]
        back = HpackModel()
        assert [(s, es, back.table.decode_block(b)) for s, es, b in deframe(out[i][0])] == sent, i
        assert back.table.entries == hes[i].model.table.entries == hhs[i].model.table.entries, i
    _close(hhs + hes)


def test_refusals(gpu):
    import ctypes as C
    from grpc_rdma_amd import h2dev
    hs = [HE(gpu) for _ in range(3)]
    encode_batch(hs, [0, 1, 2], lists={i: [(1, 0, fill(2 + i))] for i in range(3)})
    inp = Input(gpu, *pack([(3, 0, fill(4))]))
    for h in hs:
        h.set_peer(300)
        h.out = Wire(gpu, 256, 4)
    spare = Wire(gpu, 256, 4)

    def item(k, wire=None):
        wp, wc, bp, bc = (wire or hs[k].out).args()
        return (hs[k].enc,) + inp.args() + (wp, wc, bp, bc)

    misaligned = (hs[1].enc,) + inp.args() + (spare.wire.ptr + 8, 200, spare.bw.ptr, 4)
    cases = [("none", lambda: [], "BATCH_MAX"), ("257 items", lambda: [item(0)] * 257, "BATCH_MAX"),
             ("no encoder", lambda: [item(0), (None,) + inp.args() + spare.args(), item(2)], "no encoder"),
             ("twice", lambda: [item(0), item(1), item(0, spare)], "twice"),
             ("a misaligned wire arena", lambda: [item(0), misaligned, item(2)], "null, zero or misaligned"),
             ("no item array", None, None), ("no result array", None, None)]
    for what, items, why in cases:
        if items is None:
            arr, out = (h2dev.H2HpencItem * 1)(), (C.c_uint64 * 8)()
            (arr[0].enc, arr[0].d_blocks, arr[0].nblocks, arr[0].d_fields, arr[0].nfields, arr[0].d_strings, arr[0].strings_bytes, arr[0].d_wire,
             arr[0].wire_cap, arr[0].d_block_wire, arr[0].block_wire_cap) = (hs[0].enc.h,) + item(0)[1:]
            rc = h2dev.load().grdma_h2_hpenc_encode_batch(*((None, 1, out) if what == "no item array" else (arr, 1, None)))
            same(rc, INVALID, what)
        else:
            with pytest.raises(gpu.GrdmaError, match=ERR2) as e:
                h2dev.encode_batch(items())
            assert why in str(e.value), (what, str(e.value))
        unchanged(hs, what)
        data = spare.wire.read() + spare.bw.read()
        same(data, bytes([0xA5]) * len(data), what + ": nothing written")
    # nothing ran, nothing changed: the next call is exact, the pending size update included
    count, out = encode_batch(hs, [2, 0, 1], device={i: (inp.args(), pack([(3, 0, fill(4))])) for i in range(3)})
    assert count == 3 and all(out[i][0][9:12] == enc_int(300, 5, 0x20) for i in range(3)) and [_calls(h) for h in hs] == [2, 2, 2]
    _close(hs)
