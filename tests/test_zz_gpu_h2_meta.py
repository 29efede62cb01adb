"""Call metadata: decoded header blocks read on the device into call records and rejection blocks (grdma_h2_meta,
csrc/grdma_h2_meta.h).  The expected values come from the MetaModel of tests/h2_meta_model.py: the rules of
include/grdma_amd.h ("Call metadata").  Every comparison is exact (MH of tests/h2_meta_lib.py runs a call on the device
and in the model and compares the record table and the rejection list whole -- what is not written keeps its fill --
the result block and the counters); what a test asserts beside that is what the case is about.  The shapes are the
kernels' edges: the blocks a workgroup takes, the 64 fields of a step, the method table's probes."""
import pytest

from tests.h2_hpenc_lib import ERR2, HE, Input
from tests.h2_hpenc_model import pack
from tests.h2_meta_lib import (MH, PATH, PATH_COLLISION, Out, customs, encoding, flags, kind, request, response, timeout, trailers,
                               verdict)
from tests.h2_meta_model import (BAD_CONTENT_TYPE, BAD_ENCODING, BAD_GRPC_STATUS, BAD_INPUT, BAD_METHOD, BAD_TE, BAD_TIMEOUT, END_STREAM,
                                 ERR_FIELD_RANGE, ERR_STREAM, ERR_STRING, HAS_GRPC_STATUS, HAS_MESSAGE, HAS_TIMEOUT, HTTP_STATUS,
                                 KNOWN_KEYS, MALFORMED, NO_STATUS, NONE, OK, REQUEST, RESPONSE, TRAILERS, UNIMPLEMENTED)

pytestmark = pytest.mark.gpu

WG_BLOCKS, GRID, EMU_GRID = 8, 64, 2  # H2M_WG_BLOCKS, H2M_GRID of csrc/grdma_h2_meta.h on the device and under the emulator


def one(h, hs, stream=1, fl=0):
    """one block of one call -> its record"""
    recs, rej, res = h.read([(stream, fl, hs)])
    return recs[0]


# ---- block counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, WG_BLOCKS - 1, WG_BLOCKS, WG_BLOCKS + 1, EMU_GRID * WG_BLOCKS + 1, GRID * WG_BLOCKS + 3])
def test_block_counts_around_a_workgroups_run(gpu, n):
    h = MH(gpu)
    # requests, every other one to a path nobody registered: the rejections cross the runs
    recs, rej, res = h.read([(2 * k + 1, 0, request(PATH if k % 2 else b"/svc/none")) for k in range(n)])
    assert res[:2] == (n, n) and res[4] == (n + 1) // 2 and [r[0] for r in rej] == [4 * k + 1 for k in range((n + 1) // 2)]
    h.close()


# ---- fields per block ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_fields_per_block(gpu, n):
    h = MH(gpu)
    # the request's own six fields last, behind the custom ones: its pseudo-headers come late, the first of them offends
    lists = [(1, 0, [] if n == 0 else [(b"te", b"trailers")] if n == 1 else customs(n - 6) + request())]
    if n == 257:
        lists.append((3, 1, trailers()))  # beside a block of one field
    recs, rej, res = h.read(lists)
    if n < 2:
        assert (kind(recs[0]), verdict(recs[0]), recs[0][10]) == (TRAILERS, OK, 0)
    else:
        assert (kind(recs[0]), verdict(recs[0]), recs[0][10], recs[0][11], recs[0][7]) == (REQUEST, MALFORMED, n - 6, n - 6, n - 4)
    if n == 257:
        assert kind(recs[1]) == TRAILERS and verdict(recs[1]) == OK and recs[1][4] == 0
    h.close()


def test_a_long_good_request(gpu):
    h = MH(gpu)
    r = one(h, request(grpc_timeout=b"5S") + customs(300) + [(b"grpc-encoding", b"identity")])
    assert (kind(r), verdict(r), r[2], r[10], timeout(r)) == (REQUEST, OK, 0, 300, 5 * 10**9) and flags(r) == HAS_TIMEOUT
    from grpc_rdma_amd import h2dev
    view = h2dev.CallMetadata.records(h.last_out.meta.read(48))  # the device's bytes as the numpy dtype
    assert (int(view["stream"][0]), int(view["ncustom"][0]), int(view["path_field"][0]), int(view["timeout_lo"][0])) == (1, 300, 2, 5 * 10**9 & 0xffffffff)
    h.close()


# ---- the edges of a step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [1, 63, 64, 65, 128])
def test_a_pseudo_header_behind_a_regular_field(gpu, at):
    h = MH(gpu)
    r = one(h, customs(at) + request())  # (the regular field at lane 0, the first pseudo-header at `at`)
    assert verdict(r) == MALFORMED and r[11] == at and kind(r) == REQUEST and r[2] == 0 and r[7] == at + 2
    h.close()


@pytest.mark.parametrize("first, second", [(0, 1), (0, 63), (0, 64), (0, 70), (10, 70), (63, 64), (64, 128)])
def test_a_path_twice_the_first_is_the_records(gpu, first, second):
    """(Sixty-two legal fields cannot lie between two pseudo-headers: where the two stand in different steps, regular
    fields lie between them, and the second is late as well as double -- one field, one fault either way.)"""
    h = MH(gpu)
    r = one(h, customs(first) + [(b":path", PATH)] + customs(second - first - 1) + [(b":path", b"/svc/none")])
    assert (verdict(r), r[7], r[2], r[11]) == (MALFORMED, first, 0, first if first else second)
    h.close()


@pytest.mark.parametrize("gap", [0, 5, 62, 63, 64, 200])
def test_the_first_timeout_wins(gpu, gap):
    h = MH(gpu)
    r = one(h, request() + [(b"grpc-timeout", b"7m")] + customs(gap) + [(b"grpc-timeout", b"bad")])
    assert (verdict(r), timeout(r), flags(r)) == (OK, 7 * 10**6, HAS_TIMEOUT)
    r = one(h, request() + [(b"grpc-timeout", b"bad")] + customs(gap) + [(b"grpc-timeout", b"7m")])
    assert (verdict(r), timeout(r), flags(r)) == (BAD_TIMEOUT, 0, 0)
    h.close()


# ---- field legality and key lookup ----------------------------------------------------------------------------------------------
def test_each_known_key_and_its_neighbours(gpu):
    h = MH(gpu)
    lists = []
    for k, name in enumerate(KNOWN_KEYS):
        last = name[:-1] + (b"x" if name[-1:] != b"x" else b"y")
        first = (b"x" if name[:1] != b"x" else b"y") + name[1:]
        lists += [(6 * k + 1, 0, [(name, b"v")]), (6 * k + 3, 0, [(last, b"v")]), (6 * k + 5, 0, [(first, b"v")])]
    recs, rej, res = h.read(lists)
    for k, name in enumerate(KNOWN_KEYS):
        assert [r[10] for r in recs[3 * k:3 * k + 3]] == [0, 1, 1], name  # both neighbours are custom
        # a pseudo-header's neighbour in the last byte still starts with ':': a bad field; the others are plain names
        assert [verdict(r) == MALFORMED and r[11] != NONE for r in recs[3 * k + 1:3 * k + 3]] == [name[:1] == b":", False], name
    assert [verdict(r) for r in recs[0:15:3]] == [MALFORMED] * 5      # a lone pseudo-header: a request without the others, or :status v
    assert [verdict(recs[3 * k]) for k in range(12, 17)] == [MALFORMED] * 5  # the connection-specific names
    h.close()


@pytest.mark.parametrize("name", [b"x-plain", b"x-plain-bin"])
def test_every_byte_value_in_a_value(gpu, name):
    h = MH(gpu)
    recs, rej, res = h.read([(2 * b + 1, 0, [(name, b"a" + bytes([b]) + b"z")]) for b in range(256)])
    legal = [name.endswith(b"-bin") or 0x20 <= b <= 0x7e for b in range(256)]
    assert [verdict(r) == OK for r in recs] == legal and [r[11] == NONE for r in recs] == legal and res[5] == legal.count(False)
    h.close()


def test_every_byte_value_in_a_name(gpu):
    h = MH(gpu)
    recs, rej, res = h.read([(2 * b + 1, 0, [(b"x" + bytes([b]) + b"z", b"v")]) for b in range(256)])
    legal = [bytes([b]) in b"abcdefghijklmnopqrstuvwxyz0123456789-_." for b in range(256)]
    assert [verdict(r) == OK for r in recs] == legal and all(r[10] == 1 for r in recs)
    recs, rej, res = h.read([(1, 0, [(b"", b"v")]), (3, 0, [(b":", b"v")]), (5, 0, [(b"a:b", b"v")]), (7, 0, [(b"te", b"gzip")]),
                             (9, 0, [(b"te", b"trailers")])])
    assert [verdict(r) for r in recs] == [MALFORMED] * 4 + [OK]
    h.close()


# ---- the method table -----------------------------------------------------------------------------------------------------------
def test_no_method_and_one(gpu):
    h = MH(gpu, methods=())
    assert verdict(one(h, request())) == UNIMPLEMENTED
    h.close()
    h = MH(gpu, methods=(PATH,))
    recs, rej, res = h.read([(1, 0, request()), (3, 0, request(PATH[:-1] + b"N")), (5, 0, request(PATH + b"M")), (7, 0, request(PATH[:-1]))])
    assert [(verdict(r), r[2]) for r in recs] == [(OK, 0)] + [(UNIMPLEMENTED, NONE)] * 3
    h.close()


def test_4096_methods_and_the_last_one(gpu):
    methods = [b"/svc%d/M%d" % (i % 7, i) for i in range(4096)]
    h = MH(gpu, methods=methods)
    recs, rej, res = h.read([(1, 0, request(methods[-1])), (3, 0, request(methods[0])), (5, 0, request(methods[2048])),
                             (7, 0, request(b"/svc0/M4096"))])
    assert [r[2] for r in recs] == [4095, 0, 2048, NONE]
    h.close()


def test_two_paths_with_one_hash(gpu):
    a, b = PATH_COLLISION
    for methods in ((a, b), (b, a), (a,)):
        h = MH(gpu, methods=methods)
        recs, rej, res = h.read([(1, 0, request(a)), (3, 0, request(b))])
        assert [r[2] for r in recs] == [methods.index(p) if p in methods else NONE for p in (a, b)]
        h.close()


def test_the_longest_path(gpu):
    long = b"/" + b"p" * 1023
    h = MH(gpu, methods=(PATH, long))
    recs, rej, res = h.read([(1, 0, request(long)), (3, 0, request(long + b"p")), (5, 0, request(long[:-1] + b"q"))])
    assert [r[2] for r in recs] == [1, NONE, NONE]
    h.close()


# ---- verdicts -------------------------------------------------------------------------------------------------------------------
def test_every_verdict_from_a_minimal_block(gpu):
    h = MH(gpu, accept=("identity", "gzip"))
    cases = [
        (request(), 0, REQUEST, OK),
        (request(drop=(b":scheme",)), 0, REQUEST, MALFORMED),
        (request(p_scheme=b"ftp"), 0, REQUEST, MALFORMED),
        (request(path=b""), 0, REQUEST, MALFORMED),
        (request(p_method=b"GET"), 0, REQUEST, BAD_METHOD),
        (request(content_type=b"text/html"), 0, REQUEST, BAD_CONTENT_TYPE),
        (request(drop=(b"content-type",)), 0, REQUEST, BAD_CONTENT_TYPE),
        (request(drop=(b"te",)), 0, REQUEST, BAD_TE),
        (request(grpc_timeout=b"1x"), 0, REQUEST, BAD_TIMEOUT),
        (request(b"/svc/none"), 0, REQUEST, UNIMPLEMENTED),
        (request(grpc_encoding=b"snappy"), 0, REQUEST, BAD_ENCODING),
        (request(grpc_encoding=b"deflate"), 0, REQUEST, BAD_ENCODING),
        (request(grpc_encoding=b"gzip"), 0, REQUEST, OK),
        (response(b"503"), 0, RESPONSE, HTTP_STATUS),
        (response(), 0, RESPONSE, OK),
        (response(content_type=None), 0, RESPONSE, BAD_CONTENT_TYPE),
        (response(), 1, RESPONSE, NO_STATUS),
        (response(extra=trailers(b"0")), 1, RESPONSE, OK),          # Trailers-Only
        (response(extra=trailers(b"12", [(b"grpc-message", b"no")])), 1, RESPONSE, OK),
        (trailers(), 1, TRAILERS, OK),
        (trailers(None), 1, TRAILERS, NO_STATUS),
        (trailers(None), 0, TRAILERS, OK),
        (trailers(b"1234"), 1, TRAILERS, BAD_GRPC_STATUS),
        (trailers(b"1x"), 1, TRAILERS, BAD_GRPC_STATUS),
        (trailers(b"", [(b"grpc-timeout", b"")]), 1, TRAILERS, BAD_TIMEOUT),  # (the order: the timeout in front of the status)
        (request(p_method=b"GET", content_type=b"text/html", drop=(b"te",)), 0, REQUEST, BAD_METHOD),
        (request(b"/svc/none", grpc_timeout=b"S"), 0, REQUEST, BAD_TIMEOUT),
    ]
    recs, rej, res = h.read([(2 * k + 1, fl, hs) for k, (hs, fl, _, _) in enumerate(cases)])
    assert [(kind(r), verdict(r)) for r in recs] == [(k, v) for _, _, k, v in cases]
    assert encoding(recs[10]) == 255 and encoding(recs[11]) == 2 and encoding(recs[12]) == 1
    assert flags(recs[18]) == END_STREAM | HAS_GRPC_STATUS | HAS_MESSAGE and recs[18][3:5] == (200, 12) and recs[18][9] != NONE
    assert recs[13][3] == 503 and recs[22][4] == NONE and flags(recs[22]) == END_STREAM | HAS_GRPC_STATUS
    h.close()


def test_statuses_that_are_no_three_digits(gpu):
    h = MH(gpu)
    recs, rej, res = h.read([(1, 0, response(b"20")), (3, 0, response(b"2000")), (5, 0, response(b"2x0")), (7, 0, response(b"200")),
                             (9, 0, [(b":status", b"200")] + request()), (11, 0, request() + [(b":status", b"2x0")]),
                             (13, 0, [(b":status", b"2x0"), (b":method", b"POST")])])
    assert [(verdict(r), r[3], r[11]) for r in recs[:4]] == [(MALFORMED, NONE, 0), (MALFORMED, NONE, 2), (MALFORMED, NONE, 4), (OK, 200, NONE)]
    # :status beside :method: a request, malformed at the later of the two (a regular field in front offends earlier)
    assert [(kind(r), verdict(r)) for r in recs[4:]] == [(REQUEST, MALFORMED)] * 3
    assert recs[4][11] - recs[4][7] == -2 and recs[5][11] - recs[5][7] == 4 and recs[6][11] == recs[5][11] + 2
    h.close()


# ---- blocks that share fields ---------------------------------------------------------------------------------------------------------
def test_two_blocks_over_one_field_range(gpu):
    h = MH(gpu)
    blocks, fields, arena = pack([(1, 0, request(b"/svc/none"))])
    n = len(fields)
    recs, rej, res = h.read(raw=([(1, 0, n, 0), (9, 0, n, 0), (5, 2, n - 2, 0)], fields, arena))
    assert [r[0] for r in rej] == [1, 9] and recs[0][1:] == recs[1][1:] and verdict(recs[2]) == MALFORMED and kind(recs[2]) == REQUEST
    h.close()


# ---- rejections -------------------------------------------------------------------------------------------------------------------------
def test_300_requests_every_third_refused(gpu):
    h = MH(gpu, accept=("identity", "deflate"))
    refusals = [request(p_method=b"PUT"), request(content_type=b"application/json"), request(drop=(b"te",)), request(grpc_timeout=b"123456789S"),
                request(b"/svc/none"), request(grpc_encoding=b"gzip")]
    recs, rej, res = h.read([(2 * k + 1, k & 1, refusals[k // 3 % 6] if k % 3 == 0 else request()) for k in range(300)])
    assert res[:6] == (300, 300, 0, 0, 100, 0) and [r[0] for r in rej] == [6 * k + 1 for k in range(100)]
    lists = h.model.reject_lists
    assert [r[1:3] for r in rej[:6]] == [lists[v] for v in (BAD_METHOD, BAD_CONTENT_TYPE, BAD_TE, BAD_TIMEOUT, UNIMPLEMENTED, BAD_ENCODING)]
    h.close()


def test_all_refused_none_refused_and_a_malformed_one_between(gpu):
    h = MH(gpu)
    recs, rej, res = h.read([(2 * k + 1, 0, request(b"/svc/none")) for k in range(20)])
    assert res[4] == 20
    recs, rej, res = h.read([(2 * k + 1, 0, request()) for k in range(20)] + [(41, 1, trailers()), (43, 0, response(b"404"))])
    assert (res[4], rej) == (0, []) and verdict(recs[-1]) == HTTP_STATUS  # (a response is never answered)
    recs, rej, res = h.read([(1, 0, request(drop=(b"te",))), (3, 0, request(drop=(b":path",))), (5, 0, request(p_method=b"GET"))])
    assert [r[0] for r in rej] == [1, 5] and res[4:6] == (2, 1) and recs[1][11] == NONE
    h.close()


# ---- caps and bad input -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["meta", "reject"])
def test_a_cap_too_small_writes_nothing_and_the_repeat_is_exact(gpu, short):
    h = MH(gpu)
    lists = [(2 * k + 1, 0, request(PATH if k % 2 else b"/svc/none")) for k in range(21)]
    before = h.dev.stats()
    recs, rej, res = h.read(lists, meta_cap=20 if short == "meta" else 21, reject_cap=10 if short == "reject" else 11)
    assert res == (21, 21, 0, 0, 11, 0, 0, 1) and recs == [] and h.dev.stats()["calls"] == before["calls"]
    recs, rej, res = h.read(lists, meta_cap=21, reject_cap=11)  # (exactly the need: nothing is written behind the totals)
    assert res[7] == 0 and len(recs) == 21 and len(rej) == 11
    h.close()


def test_bad_input_names_the_block(gpu):
    h = MH(gpu)
    blocks, fields, arena = pack([(2 * k + 1, 0, request()) for k in range(12)])
    n = len(fields) // 12

    def word(raw):
        return h.read(raw=raw)[2][6]

    for k in (0, 5, 11):
        bad = list(blocks)
        bad[k] = (bad[k][0], bad[k][1], len(fields) - bad[k][1] + 1, 0)
        assert word((bad, fields, arena)) == BAD_INPUT | ERR_FIELD_RANGE << 8 | k << 32
        for sid in (0, 1 << 31):
            bad = list(blocks)
            bad[k] = (sid,) + bad[k][1:]
            assert word((bad, fields, arena)) == BAD_INPUT | ERR_STREAM << 8 | k << 32
        for which in (0, 1):
            bad = list(fields)
            f = bad[k * n + 3]
            bad[k * n + 3] = (len(arena) - (f[2] & 0xffffff) + 1, f[1], f[2], f[3]) if which == 0 else (f[0], len(arena), f[2], 1)
            assert word((blocks, bad, arena)) == BAD_INPUT | ERR_STRING << 8 | k << 32
    # the first block with a fault; in it the range in front of the stream in front of the strings; a hint is no length
    bad = list(blocks)
    bad[7], bad[3] = (0,) + bad[7][1:], (0, bad[3][1], len(fields), 0)
    assert word((bad, fields, arena)) == BAD_INPUT | ERR_FIELD_RANGE << 8 | 3 << 32
    assert word((blocks, [(a, b, c | 0xff << 24, d) for a, b, c, d in fields], arena)) == 0
    # a string that leaves the arena in a field no block holds is nobody's fault
    assert word((blocks[:11], fields[:11 * n] + [(len(arena), 0, 1, 0)] * n, arena)) == 0
    assert h.dev.stats()["calls"] == 2  # (not sticky, and a refused call counts nowhere)
    h.close()


def test_refusals_and_lifetime(gpu):
    from grpc_rdma_amd import h2dev
    lib = h2dev.load()
    dump = lambda ms: b"".join(len(m).to_bytes(4, "little") + m for m in ms)  # noqa: E731
    good = dump([b"/a", b"/b"])
    for args in ((dump([b"/a", b"/a"]), 12, 2, 1), (good, len(good) + 1, 2, 1), (good, len(good) - 1, 2, 1), (good, len(good), 1, 1),
                 (good, len(good), 3, 1), (dump([b""]), 4, 1, 1), (dump([b"/" * 1025]), 1029, 1, 1), (good, len(good), 2, 8 | 1), (good, len(good), 2, 2),
                 (good, len(good), 2, 0), (None, 0, 4097, 1)):
        assert not lib.grdma_h2_meta_create(*args) and lib.grdma_last_error()
    with pytest.raises(gpu.GrdmaError):
        h2dev.CallMetadata(methods=[b"/a", b"/a"])
    h = MH(gpu)
    inp = Input(gpu, *pack([(1, 0, request())]))
    o = Out(gpu, 4, 4)
    mp, mc, rp, rc = o.args()
    for targets in ((0, mc, rp, rc), (mp, 0, rp, rc), (mp, mc, 0, rc), (mp, mc, rp, 0), (mp + 8, mc, rp, rc), (mp, mc, rp + 8, rc)):
        with pytest.raises(gpu.GrdmaError, match=ERR2):
            h.dev.read(*inp.args(), *targets)
    bp, nb, fp, nf, sp, ns = inp.args()
    for tables in ((0, nb, fp, nf, sp, ns), (bp, nb, 0, nf, sp, ns), (bp, nb, fp, nf, 0, ns), (bp + 8, nb, fp, nf, sp, ns), (bp, nb, fp + 8, nf, sp, ns),
                   (bp, 0xffffffff, fp, nf, sp, ns)):
        with pytest.raises(gpu.GrdmaError, match=ERR2):
            h.dev.read(*tables, mp, mc, rp, rc)
    assert lib.grdma_h2_meta_read(h.dev.h, bp, nb, fp, nf, sp, ns, mp, mc, rp, rc, None) == -2  # no result array
    assert lib.grdma_h2_meta_read(None, bp, nb, fp, nf, sp, ns, mp, mc, rp, rc, None) == -2     # no reader
    assert o.meta.read() == bytes([0xA5]) * (48 * 6) and o.reject.read() == bytes([0xA5]) * (16 * 8)
    h.read([(1, 0, request())])  # nothing of that changed anything
    other = MH(gpu, methods=(b"/other",), accept=("identity", "gzip", "deflate"))  # a second reader beside the first
    assert verdict(one(other, request())) == UNIMPLEMENTED and verdict(one(h, request())) == OK
    h.close()
    h.close()
    assert verdict(one(other, request(b"/other", grpc_encoding=b"deflate"))) == OK
    other.close()
    for _ in range(3):  # create and destroy with a call in between
        x = MH(gpu)
        x.read([(1, 0, request())])
        x.close()


# ---- decode, read, encode: end to end on the device ------------------------------------------------------------------------------------------
def test_decode_read_and_encode_the_rejections(gpu):
    from tests.h2_hpack_lib import HH, headers_frames, literal
    calls = [(1, request()), (3, request(b"/svc/none")), (5, request(p_method=b"GET")), (7, request(drop=(b":scheme",))),
             (9, request(grpc_encoding=b"gzip")), (11, request(grpc_timeout=b"10S")), (13, request(drop=(b"te",))),
             (15, request(content_type=b"text/plain")), (17, request(grpc_timeout=b"10"))]
    expected = {3: (b"200", b"12"), 5: (b"405", b"13"), 9: (b"200", b"12"), 13: (b"400", b"13"), 15: (b"415", b"13"), 17: (b"400", b"13")}
    dec, m, enc, back = HH(gpu), MH(gpu), HE(gpu), HH(gpu)
    words = lambda data, n: [tuple(int.from_bytes(data[16 * i + 4 * j:16 * i + 4 * j + 4], "little") for j in range(4)) for i in range(n)]  # noqa: E731
    fp, nf, sp, ns = m.dev.reject_tables()
    for again in (False, True):
        base = 100 if again else 0  # (new streams: the first call's are closed)
        wire = b"".join(headers_frames(base + sid, b"".join(literal(n, v, 2) for n, v in hs), flags=1) for sid, hs in calls)
        lists, res = dec.feed([wire])
        t = dec.target
        raw = tuple(x.read() for x in (t.blocks, t.fields, t.strings))
        # the decoder's three device targets are the reader's input; the reader's rejection list and its constant tables
        # are the encoder's: no table passes through the host (the reads around them are the test's comparisons)
        recs, rej, mres = m.read(raw=(words(raw[0], res[0]), words(raw[1], res[1]), raw[2][:res[2]]),
                                 device=(t.blocks.ptr, res[0], t.fields.ptr, res[1], t.strings.ptr, res[2]))
        assert [r[0] - base for r in rej] == sorted(expected) and mres[5] == 1
        out, bw, eres = enc.encode(raw=(rej, m.model.reject_fields, m.model.reject_arena),
                                   device=(m.last_out.reject.ptr, len(rej), fp, nf, sp, ns))
        got, _ = back.feed([out])
        assert [sid - base for sid, _, _ in got] == sorted(expected) and all(fl & 1 for _, fl, _ in got)
        for sid, _, hs in got:
            d = {n: v for n, v, _ in hs}
            assert (d[b":status"], d[b"grpc-status"]) == expected[sid - base] and d[b"content-type"] == b"application/grpc" and d[b"grpc-message"]
            assert (b"grpc-accept-encoding" in d) == (sid - base == 9) and d.get(b"grpc-accept-encoding", b"identity") == b"identity"
        if again:  # everything the lists hold is in the peer's table by now: one byte a field
            assert [ln - 9 for _, ln, _ in bw] == [r[2] for r in rej] and eres[3] == 0
    for x in (dec, m, enc, back):
        x.close()
