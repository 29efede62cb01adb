"""Call metadata on many links: the decoder output of a table of links read through ONE reader in the same three launches
(k_h2_links_meta_*, grdma_h2_meta_read_batch, CallMetadata.read_batch).  Every item of a batch is compared exactly with
the reader's one MetaModel (tests/h2_meta_model.py), stepped per item in item order, through read_batch of
tests/h2_links_meta_lib.py: the result tuple, the record table and the rejection list whole, and the reader's counters,
which move by ONE call and by the sums over the items read.  The point is the link indexing, a link's share of the grid
(four workgroups, two under the emulator), the per-item outcomes and the one count -- not the reader's rules
(tests/test_zz_gpu_h2_meta.py)."""
import random

import pytest

from tests.h2_device_lib import same
from tests.h2_hpenc_lib import ERR2
from tests.h2_hpenc_model import pack
from tests.h2_links_meta_lib import MH, Input, Out, compare, prepare, read_batch, unchanged
from tests.h2_meta_lib import PATH, customs, kind, request, response, trailers, verdict
from tests.h2_meta_model import (BAD_INPUT, ERR_FIELD_RANGE, ERR_STREAM, ERR_STRING, MALFORMED, OK, REQUEST, STAT_KEYS, TRAILERS,
                                 UNIMPLEMENTED, MetaModel)

pytestmark = pytest.mark.gpu

INVALID = -2  # -GRDMA_ERR_INVALID
NOWHERE = b"/svc/none"
SMALL = [(1, 0, request())]                       # a trivially small link: one good request
SMALL_REFUSED = [(1, 0, request(NOWHERE))]        # ... and one with a rejection of its own


def mixed(n, refused=(), malformed=(), first=1):
    """n requests on the streams first, first + 2, ...: those at the positions of `refused` name no method, those at
    `malformed` lack :path, the others are good"""
    return [(first + 2 * k, k & 1, request(NOWHERE) if k in refused else request(drop=(b":path",)) if k in malformed else request())
            for k in range(n)]


def counters(h):
    st = h.dev.stats()
    return tuple(st[k] for k in STAT_KEYS)


# ---- shapes a link can go wrong at: the shape under test between two trivially small links --------------------------------------
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 24, 25, 32, 33, 64, 65, 129, 1025])
def test_blocks_in_a_link(gpu, n):
    # (the 8-block run, the fourth workgroup, `per` above 8, a wave's second trip above 16 blocks a run, the emit's
    # second scan step above 256 blocks a run)
    h = MH(gpu)
    refused = set(range(0, n, 3))
    malformed = set(range(1, n, 7)) - refused
    count, out, _ = read_batch(h, [0, 1, 2], lists={0: SMALL_REFUSED, 1: mixed(n, refused, malformed), 2: SMALL})
    nrej, nmal = len(refused), len(malformed)
    assert count == 3 and out[1][2] == (n, n, 0, 0, nrej, nmal, 0, 0)
    assert out[0][2][4] == 1 and out[2][2] == (1, 1, 0, 0, 0, 0, 0, 0) and counters(h) == (1, n + 2, n + 2, 0, 0, nrej + 1, nmal)
    h.close()


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_fields_in_a_link(gpu, n):
    # (the fields stage's stride at four workgroups of 256 lanes: one field short of it, exactly it, one more)
    h = MH(gpu)
    lists = [(2 * k + 1, 0, request() + customs(250)) for k in range(3)] + [(7, 1, request(NOWHERE) + customs(n - 768 - 6))]
    same(len(pack(lists)[1]), n, "the link's fields")
    count, out, _ = read_batch(h, [0, 1, 2], lists={0: SMALL, 1: lists, 2: SMALL_REFUSED})
    assert count == 3 and out[1][2] == (4, 4, 0, 0, 1, 0, 0, 0) and out[1][0][3][10] == n - 768 - 6 and verdict(out[1][0][3]) == UNIMPLEMENTED
    h.close()


def test_a_block_whose_first_known_key_is_in_the_second_step(gpu):
    h = MH(gpu)
    lists = [(1, 1, customs(64) + trailers(b"7")), (3, 0, customs(64) + [(b"te", b"trailers")] + request(drop=(b"te",)))]
    count, out, _ = read_batch(h, [0, 1, 2], lists={0: SMALL, 1: lists, 2: SMALL})
    recs = out[1][0]
    assert count == 3 and (kind(recs[0]), verdict(recs[0]), recs[0][4], recs[0][10]) == (TRAILERS, OK, 7, 64)
    assert (kind(recs[1]), verdict(recs[1]), recs[1][11]) == (REQUEST, MALFORMED, 65 + 65)  # (:method behind regular fields)
    h.close()


# ---- the rejection list ----------------------------------------------------------------------------------------------------------
def test_compaction_stays_inside_its_link(gpu):
    # 40 blocks: a run is 10 blocks (20 under the emulator); 36 blocks: 9 (18).  Rejections on both sides of every border,
    # a malformed request between refused ones; one neighbour all refused, one none
    h = MH(gpu)
    a = mixed(40, refused=(0, 9, 10, 14, 16, 19, 20, 29, 30, 39), malformed=(15,))
    b = mixed(36, refused=(8, 9, 17, 18, 26, 27, 35), malformed=(0, 16), first=101)
    lists = {0: mixed(40, refused=range(40), first=201), 1: a, 2: mixed(40), 3: b, 4: mixed(16, refused=range(16), first=301)}
    count, out, _ = read_batch(h, [0, 1, 2, 3, 4], lists=lists)
    assert count == 5 and [out[i][2][4] for i in range(5)] == [40, 10, 0, 7, 16]
    assert [r[0] for r in out[1][1]] == [1 + 2 * k for k in (0, 9, 10, 14, 16, 19, 20, 29, 30, 39)]
    assert [r[0] for r in out[3][1]] == [101 + 2 * k for k in (8, 9, 17, 18, 26, 27, 35)] and out[3][2][5] == 2
    assert [r[0] for r in out[4][1]] == [301 + 2 * k for k in range(16)] and counters(h)[5:] == (73, 3)
    h.close()


def test_batch_against_single_on_twin_readers(gpu):
    a, b = MH(gpu, accept=("identity", "gzip")), MH(gpu, accept=("identity", "gzip"))
    lists = {0: mixed(21, refused=(0, 7, 20)), 1: [(1, 0, response()), (1, 1, trailers()), (3, 0, request(grpc_encoding=b"deflate"))],
             2: mixed(9, malformed=(4,)) + [(99, 1, response(b"404"))], 3: []}
    order = [2, 0, 3, 1]
    count, out, links = read_batch(b, order, lists=lists)
    assert count == 4
    for i in order:
        single = a.read(lists[i])
        assert single == out[i], i
        same(links[i].out.meta.read(), a.last_out.meta.read(), "item %d: twin record tables" % i)
        same(links[i].out.reject.read(), a.last_out.reject.read(), "item %d: twin rejection lists" % i)
    # the batch is ONE call; every other counter is the loop's
    assert counters(b)[0] == 1 and counters(a)[0] == 4 and counters(b)[1:] == counters(a)[1:]
    a.close()
    b.close()


def test_nine_links_in_shuffled_order_over_three_calls(gpu):
    h = MH(gpu)
    rng = random.Random(11)

    def own(i, n):
        """link i's blocks of call n: 3 i + n requests, its own positions refused and malformed, then its trailers"""
        nb = 3 * i + n
        return mixed(nb, refused=range(i % 4, nb, 4), malformed=range(i % 5 + 1, nb, 5), first=1000 * n + 1) + [(1000 * n + 999, 1, trailers(b"%d" % i))]

    total = (0,) * 7
    for n in range(3):
        order = list(range(9))
        rng.shuffle(order)
        count, out, _ = read_batch(h, order, lists={i: own(i, n) for i in range(9)})  # (compare checks the counters after the call)
        assert count == 9 and all(out[i][2][0] == 3 * i + n + 1 and out[i][2][3] == 1 and out[i][2][6:] == (0, 0) for i in range(9)), n
        total = (n + 1,) + tuple(t + sum(out[i][2][k] for i in range(9)) for k, t in enumerate(total[1:]))
        assert counters(h) == total, n
    h.close()


def test_trouble_stays_with_its_item(gpu):
    h = MH(gpu)
    blocks, fields, arena = pack(mixed(12))
    n = len(fields) // 12
    bad_range = (blocks[:5] + [(11, blocks[5][1], len(fields) - blocks[5][1] + 1, 0)] + blocks[6:], fields, arena)
    bad_stream = ([(0,) + blocks[0][1:]] + blocks[1:], fields, arena)
    f = fields[11 * n + 2]
    bad_string = (blocks, fields[:11 * n + 2] + [(f[0], len(arena), f[2], 1)] + fields[11 * n + 3:], arena)
    l3, l4 = mixed(21, refused=range(0, 21, 2)), mixed(20, refused=range(1, 20, 2), malformed=(4,), first=501)
    g5, g6 = mixed(17, refused=(3, 16), malformed=(9,)) + [(77, 1, trailers())], [(1, 0, response()), (3, 0, request(NOWHERE))]
    before = counters(h)
    count, out, links = read_batch(h, [5, 3, 0, 6, 1, 4, 2], raw={0: bad_range, 1: bad_stream, 2: bad_string},
                                   lists={3: l3, 4: l4, 5: g5, 6: g6}, caps={3: (20, None), 4: (None, 9)})
    assert count == 2  # exactly the two good items
    assert out[0][2] == (0, 0, 0, 0, 0, 0, BAD_INPUT | ERR_FIELD_RANGE << 8 | 5 << 32, 0)
    assert out[1][2] == (0, 0, 0, 0, 0, 0, BAD_INPUT | ERR_STREAM << 8 | 0 << 32, 0)
    assert out[2][2] == (0, 0, 0, 0, 0, 0, BAD_INPUT | ERR_STRING << 8 | 11 << 32, 0)
    assert out[3][2] == (21, 21, 0, 0, 11, 0, 0, 1) and out[4][2] == (20, 20, 0, 0, 10, 1, 0, 1)
    assert out[5][2] == (18, 17, 0, 1, 2, 1, 0, 0) and out[6][2] == (2, 1, 1, 0, 1, 0, 0, 0)
    for i in range(5):  # (compare held the five to their fill already: here it is said once more, by itself)
        for buf in (links[i].out.meta, links[i].out.reject):
            data = buf.read()
            same(data, bytes([0xA5]) * len(data), "item %d holds nothing but its fill" % i)
    assert counters(h) == (before[0] + 1, 20, 18, 1, 1, 3, 1)  # the two good items alone, in ONE call
    # the two overflowed items again, with room, in a later batch: what a never-refused model gives
    ref = MetaModel((PATH,))
    want = [ref.read(*pack(lists), 1 << 40, 1 << 40)[:3] for lists in (l3, l4)]
    count, later, _ = read_batch(h, [4, 3], lists={3: l3, 4: l4}, caps={3: (21, 11), 4: (20, 10)})  # (exactly the need)
    assert count == 2 and later[3] == tuple(want[0]) and later[4] == tuple(want[1]) and counters(h)[0] == before[0] + 2
    # a batch in which no item is read: 0, and no counter moves
    at = counters(h)
    count, out, _ = read_batch(h, [0, 3, 2], raw={0: bad_stream, 2: bad_string}, lists={3: l3}, caps={3: (21, 10)})
    assert count == 0 and out[3][2][7] == 1 and counters(h) == at
    h.close()


# ---- many items ------------------------------------------------------------------------------------------------------------------
def test_one_input_read_by_sixteen_items(gpu):
    h = MH(gpu)
    tables = pack(mixed(30, refused=range(2, 30, 5), malformed=(11,)) + [(91, 1, trailers()), (93, 0, response())])
    inp = Input(gpu, *tables)
    order = list(range(16))
    count, out, links = read_batch(h, order, device={i: (inp.args(), tables) for i in order})
    assert count == 16 and all(out[i] == out[0] for i in order) and out[0][2] == (32, 30, 1, 1, 6, 1, 0, 0)
    for i in order[1:]:
        same(links[i].out.meta.read(), links[0].out.meta.read(), "sixteen record tables")
        same(links[i].out.reject.read(), links[0].out.reject.read(), "sixteen rejection lists")
    assert counters(h) == (1, 16 * 32, 16 * 30, 16, 16, 16 * 6, 16)
    h.close()


@pytest.mark.parametrize("nlinks", [33, 256])
def test_many_links_each_with_its_own_mix(gpu, nlinks):
    # (33: one more than a power of two and more than the emulator's grid; 256: GRDMA_H2_BATCH_MAX.  Seven uploaded
    # inputs, each link one of them by its number: its own targets, its neighbours' inputs differ)
    h = MH(gpu)
    tables = [pack(mixed(3 + 5 * j, refused=range(j % 3, 3 + 5 * j, 3), malformed=range(1, 3 + 5 * j, 4 + j), first=100 * j + 1) +
                   ([(9999, 1, trailers())] if j & 1 else [])) for j in range(7)]
    inps = [Input(gpu, *t) for t in tables]
    order = list(range(nlinks))
    random.Random(nlinks).shuffle(order)
    count, out, _ = read_batch(h, order, device={i: (inps[i % 7].args(), tables[i % 7]) for i in order})
    assert count == nlinks
    for i in order:
        j = i % 7
        assert out[i] == out[j] and out[i][2][:4] == (3 + 5 * j + (j & 1), 3 + 5 * j, 0, j & 1) and out[i][2][4] and out[i][2][6:] == (0, 0), i
    assert counters(h) == (1,) + tuple(sum(out[i][2][k] for i in order) for k in range(6))
    h.close()


def test_an_empty_item_between_full_ones(gpu):
    h = MH(gpu)
    count, out, links = read_batch(h, [0, 1, 2], lists={0: mixed(10, refused=(9,)), 1: [], 2: mixed(10, refused=(0,), first=51)})
    assert count == 3 and out[1] == ([], [], (0,) * 8) and out[0][1][0][0] == 19 and out[2][1][0][0] == 51
    # ... with no tables at all, and alone
    o = Out(gpu, 1, 1)
    count, got = h.dev.read_batch([(0, 0, 0, 0, 0, 0) + o.args()])
    assert (count, got) == (1, [(0,) * 8]) and counters(h) == (2, 20, 20, 0, 0, 2, 0)
    same(o.meta.read() + o.reject.read(), bytes([0xA5]) * (48 * 3 + 16 * 5), "an empty item writes nothing")
    h.close()


# ---- decode batch, read batch, encode batch: end to end on the device ----------------------------------------------------------------
def test_device_chain_on_three_links(gpu):
    from grpc_rdma_amd import h2dev
    from tests.h2_hpack_lib import HH, headers_frames, literal
    from tests.h2_hpack_model import HpackModel
    from tests.h2_hpenc_model import deframe
    from tests.h2_links_hpack_lib import _step
    from tests.h2_links_hpenc_lib import HE
    from tests.h2_links_hpenc_lib import compare as compare_wire
    from tests.h2_links_hpenc_lib import prepare as prepare_wire
    calls = {0: [(1, request()), (3, request(NOWHERE)), (5, request(p_method=b"GET")), (7, request(drop=(b":scheme",)))],
             1: [(9, request(grpc_encoding=b"gzip")), (11, request(grpc_timeout=b"10S"))],
             2: [(13, request(drop=(b"te",))), (15, request(content_type=b"text/plain")), (17, request(grpc_timeout=b"10")), (19, request())]}
    expected = {3: (b"200", b"12"), 5: (b"405", b"13"), 9: (b"200", b"12"), 13: (b"400", b"13"), 15: (b"415", b"13"), 17: (b"400", b"13")}
    hhs, m, hes = [HH(gpu, caps=(8, 64, 2048)) for _ in range(3)], MH(gpu), [HE(gpu) for _ in range(3)]
    fp, nf, sp, ns = m.dev.reject_tables()
    order = [2, 0, 1]
    for i in order:
        hhs[i].deframe([b"".join(headers_frames(sid, b"".join(literal(n, v, 2) for n, v in hs), flags=1) for sid, hs in calls[i])])
    decoded = _step(hhs, order, None, ())  # (the decoders' models: what the targets will hold)
    # 1. decode every link; the three counts of a link stand in its result block
    _, dgot = h2dev.decode_batch([(hhs[i].dec,) + hhs[i].target.args() for i in order])
    device = {}
    for k, i in enumerate(order):
        blocks, fields, strings, res = decoded[i]
        same(dgot[k], res, "decoder %d: result" % i)
        t = hhs[i].target
        device[i] = ((t.blocks.ptr, dgot[k][0], t.fields.ptr, dgot[k][1], t.strings.ptr, dgot[k][2]), ([tuple(b) for b in blocks], fields, strings))
    # 2. read every link where the decoders left it: no table passes through the host
    items, links = prepare(m, order, device=device)
    count, mgot = m.dev.read_batch(items)
    # 3. refuse on every link: the rejection lists over the reader's ONE pair of constant tables
    wire_in = {i: ((links[i].out.reject.ptr, mgot[k][4], fp, nf, sp, ns), (links[i].exp[1], m.model.reject_fields, m.model.reject_arena))
               for k, i in enumerate(order)}
    witems, wexp = prepare_wire(hes, order, device=wire_in)
    wcount, wgot = h2dev.encode_batch(witems)
    # (the comparisons, behind the three calls)
    out = compare(m, order, links, count, mgot)
    wires = compare_wire(hes, order, wexp, wcount, wgot)
    assert count == 3 and wcount == 3 and [out[i][2][4] for i in range(3)] == [2, 1, 3] and out[0][2][5] == 1
    for i in range(3):
        back = HpackModel()
        got = [(sid, es, back.table.decode_block(b)) for sid, es, b in deframe(wires[i][0])]
        assert [sid for sid, _, _ in got] == [sid for sid, _ in calls[i] if sid in expected] and all(es for _, es, _ in got), i
        for sid, _, hs in got:  # the Trailers-Only lists of rule 8
            d = {n: v for n, v, *_ in hs}
            assert (d[b":status"], d[b"grpc-status"]) == expected[sid] and d[b"content-type"] == b"application/grpc" and d[b"grpc-message"]
            assert (b"grpc-accept-encoding" in d) == (sid == 9)
    for x in hhs + [m] + hes:
        x.close()


# ---- refusals and lifetime ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime(gpu):
    import ctypes as C
    from grpc_rdma_amd import h2dev
    lib = h2dev.load()
    h = MH(gpu)
    read_batch(h, [0, 1], lists={0: SMALL, 1: SMALL_REFUSED})
    inp = Input(gpu, *pack(mixed(4, refused=(1,))))
    stats = dict(h.model.stats)
    items, links = prepare(h, [0, 1, 2], device={k: (inp.args(), pack(mixed(4, refused=(1,)))) for k in range(3)})
    h.model.stats = stats  # (prepare stepped the model for a call that is never made)
    bp, nb, fp, nf, sp, ns = inp.args()
    mp, mc, rp, rc = items[1][6:]

    def with_item(item):
        return [items[0], item, items[2]]

    gone = h2dev.CallMetadata()
    gone.close()
    cases = [("none", h.dev, [], "BATCH_MAX"), ("257 items", h.dev, [items[0]] * 257, "BATCH_MAX"), ("a closed reader", gone, items, "no reader"),
             ("a misaligned record table", h.dev, with_item(inp.args() + (mp + 8, mc, rp, rc)), "null, zero or misaligned"),
             ("a misaligned rejection list", h.dev, with_item(inp.args() + (mp, mc, rp + 8, rc)), "null, zero or misaligned"),
             ("a zero record cap", h.dev, with_item(inp.args() + (mp, 0, rp, rc)), "null, zero or misaligned"),
             ("a zero rejection cap", h.dev, with_item(inp.args() + (mp, mc, rp, 0)), "null, zero or misaligned"),
             ("no record table", h.dev, with_item(inp.args() + (0, mc, rp, rc)), "null, zero or misaligned"),
             ("no block table, four blocks", h.dev, with_item((0, nb, fp, nf, sp, ns, mp, mc, rp, rc)), "null or misaligned"),
             ("no field table, some fields", h.dev, with_item((bp, nb, 0, nf, sp, ns, mp, mc, rp, rc)), "null or misaligned"),
             ("no string arena, some bytes", h.dev, with_item((bp, nb, fp, nf, 0, ns, mp, mc, rp, rc)), "null or misaligned"),
             ("a misaligned block table", h.dev, with_item((bp + 8, nb, fp, nf, sp, ns, mp, mc, rp, rc)), "null or misaligned"),
             ("2^32 - 1 blocks", h.dev, with_item((bp, 0xffffffff, fp, nf, sp, ns, mp, mc, rp, rc)), "2^32 - 1"),
             ("no item array", None, None, "no item array"), ("no result array", None, None, "no result array")]
    for what, dev, its, why in cases:
        if dev is None:
            import numpy as np
            arr, out = np.array([items[0]], dtype="<u8"), (C.c_uint64 * 8)(*([7] * 8))
            args = (None, 1, out) if what == "no item array" else (arr.ctypes.data_as(C.c_void_p), 1, None)
            same(lib.grdma_h2_meta_read_batch(h.dev.h, *args), INVALID, what)
            same(list(out), [7] * 8, what + ": the result words are not touched")
        else:
            with pytest.raises(gpu.GrdmaError, match=ERR2):
                dev.read_batch(its)
            same(dev.last_results, [(0,) * 8] * len(its), what + ": the result words are not touched")
        assert why in lib.grdma_last_error().decode(), (what, lib.grdma_last_error())
        unchanged(h, links, what)
    # nothing ran, nothing changed: the next call is exact
    count, out, _ = read_batch(h, [1, 0], device={k: (inp.args(), pack(mixed(4, refused=(1,)))) for k in range(2)})
    assert count == 2 and out[0][2] == (4, 4, 0, 0, 1, 0, 0, 0) and counters(h)[0] == 2
    # close() directly behind a batch: the targets hold what the call wrote
    x = MH(gpu)
    items, links = prepare(x, [0, 1], lists={0: mixed(40, refused=range(0, 40, 2)), 1: SMALL})
    count, got = x.dev.read_batch(items)
    x.close()
    compare(x, [0, 1], links, count, got, counters=False)
    x.close()
    h.close()
