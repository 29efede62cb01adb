"""The model of the call-metadata reader (tests/h2_meta_model.py) against vectors written by hand from the rules of
include/grdma_amd.h, "Call metadata" (tests/golden/h2_meta_vectors.json), and its tables against the generated header
the device is built from (csrc/grdma_h2_meta_tables.h)."""
import json
import os

import pytest

from tests import h2_meta_model as M
from tests.h2_hpenc_model import hash_bytes, pack
from tests.h2_meta_lib import PATH_COLLISION, encoding, flags, kind, timeout, verdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "h2_meta_vectors.json"), encoding="utf-8"))
WORDS = {"method": 2, "http_status": 3, "grpc_status": 4, "path_field": 7, "authority_field": 8, "message_field": 9, "ncustom": 10, "bad_field": 11}
PARTS = {"kind": kind, "verdict": verdict, "encoding": encoding, "flags": flags, "timeout": timeout}


def _gen():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_h2_meta_tables", os.path.join(ROOT, "tools", "gen_h2_meta_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_the_committed_tables_header_is_what_the_generator_writes():
    """the model's known-key and rejection tables equal the generated header: the header is this text, byte for byte"""
    gen = _gen()
    text = open(gen.PATH).read()
    assert text == gen.text()
    for key in M.KNOWN_KEYS:  # (and the text does hold them: every key's bytes, every rejection string)
        assert ", ".join(str(b) for b in key) in text.replace(",\n ", ",")
    for _, status, grpc_status, message in M.REJECTIONS:
        assert '"%s", "%s", "%s"' % (status.decode(), grpc_status.decode(), message.decode()) in text


def test_the_two_numbers_of_the_saturation_edge():
    most = 2**63 - 1
    assert 2562047 * 3600 * 10**9 == 9223369200000000000 <= most < 2562048 * 3600 * 10**9 == 9223372800000000000
    assert 99999999 * 3600 * 10**9 > 2**64  # (what a 64-bit product would lose: compared before it is multiplied)
    assert M.timeout_ns(b"2562047H") == 9223369200000000000 and M.timeout_ns(b"2562048H") == most and M.timeout_ns(b"99999999H") == most
    assert all(99999999 * unit <= most for u, unit in M.UNITS.items() if u != b"H")  # only hours saturate with eight digits


@pytest.mark.parametrize("value, ns", VECTORS["timeouts"])
def test_timeouts(value, ns):
    assert M.timeout_ns(value.encode()) == ns
    rec = M.MetaModel().block(1, 0, 1, 0, *pack([(1, 0, [(b"grpc-timeout", value.encode())])])[1:])
    assert (timeout(rec), flags(rec), verdict(rec)) == ((ns, M.HAS_TIMEOUT, M.OK) if ns is not None else (0, 0, M.BAD_TIMEOUT))


def test_every_unit_is_in_the_vectors():
    assert {v[-1:] for v, ns in VECTORS["timeouts"] if ns is not None} == {u.decode() for u in M.UNITS}


@pytest.mark.parametrize("value, good", VECTORS["content_types"])
def test_content_types(value, good):
    assert M.content_type_is_good(value.encode()) == good


@pytest.mark.parametrize("v", VECTORS["blocks"], ids=lambda v: v["name"].split(":")[0].split(",")[0])
def test_blocks(v):
    m = M.MetaModel([p.encode() for p in VECTORS["methods"]], M.accept_bits(VECTORS["accept"]))
    hs = [(n.encode("latin-1"), x.encode("latin-1")) for n, x in v["headers"]]
    # (behind three fields of another block: the record's indices are the field table's)
    blocks, fields, arena = pack([(9, 1, [(b"grpc-status", b"0")] * 3), (5, int(v["end_stream"]), hs)])
    recs, rej, res, err = m.read(blocks, fields, arena, 2, 2)
    rec = recs[1]
    assert err is None and rec[0] == 5 and verdict(recs[0]) == M.OK
    for key, want in v["expect"].items():
        got = PARTS[key](rec) if key in PARTS else rec[WORDS[key]]
        if key.endswith("_field"):
            want = want + 3 if want is not None else None
        assert got == (M.NONE if want is None else want), (v["name"], key)
    assert rej == ([(5,) + m.reject_lists[verdict(rec)] + (1,)] if v["rejected"] else [])


def test_every_verdict_is_in_the_vectors():
    assert {v["expect"]["verdict"] for v in VECTORS["blocks"]} == set(range(11))
    assert {v["expect"]["verdict"] for v in VECTORS["blocks"] if v["rejected"]} == {r[0] for r in M.REJECTIONS}


def test_the_rejection_lists():
    fields, arena, lists = M.reject_tables(M.accept_bits(["identity", "deflate"]))
    want = {M.BAD_METHOD: (b"405", b"13"), M.BAD_CONTENT_TYPE: (b"415", b"13"), M.BAD_TE: (b"400", b"13"), M.BAD_TIMEOUT: (b"400", b"13"),
            M.UNIMPLEMENTED: (b"200", b"12"), M.BAD_ENCODING: (b"200", b"12")}
    assert set(lists) == set(want)
    for v, (first, n) in lists.items():
        hs = [(arena[no:no + (nl & 0xffffff)], arena[vo:vo + vl], nl >> 24) for no, vo, nl, vl in fields[first:first + n]]
        assert [h[0] for h in hs[:4]] == [b":status", b"content-type", b"grpc-status", b"grpc-message"] and all(h[2] == 1 for h in hs)
        assert (hs[0][1], hs[2][1]) == want[v] and hs[1][1] == b"application/grpc" and hs[3][1]
        assert hs[4:] == ([(b"grpc-accept-encoding", b"identity,deflate", 1)] if v == M.BAD_ENCODING else [])
        assert not any(M.field_is_bad(n, x) for n, x, _ in hs)  # (what the reader sends, the reader would take)


def test_the_colliding_paths_collide():
    a, b = PATH_COLLISION
    assert a != b and hash_bytes(a) == hash_bytes(b) == 0x95edaa02
    for methods in ([a, b], [b, a]):
        t = M.MethodTable(methods)
        assert [t.find(a), t.find(b), t.find(a + b"x")] == [methods.index(a), methods.index(b), M.NONE]
    assert M.MethodTable([a]).find(b) == M.NONE  # bytes decide


def test_the_method_table():
    assert M.MethodTable([]).nslots == 2 and M.MethodTable([]).find(b"/x") == M.NONE
    ms = [b"/s/%d" % i for i in range(4096)]
    t = M.MethodTable(ms)
    assert t.nslots == 8192 and [t.find(p) for p in (ms[0], ms[4095])] == [0, 4095] and t.find(b"/s/4096") == M.NONE
    assert M.MethodTable(ms[:3]).nslots == 8 and M.MethodTable(ms[:4]).nslots == 8 and M.MethodTable(ms[:5]).nslots == 16
    assert M.check_methods([b"/a", b"/a"], 1) and M.check_methods([b""], 1) and M.check_methods([b"/" * 1025], 1)
    assert M.check_methods([b"/a"], 2) and M.check_methods([b"/a"], 9) and M.check_methods(ms + [b"/more"], 1)
    assert M.check_methods(ms, 7) is None and M.dump_methods([b"/a", b"/bc"]) == b"\x02\0\0\0/a\x03\0\0\0/bc"


def test_the_numpy_view_of_a_record_table():
    from grpc_rdma_amd import h2dev
    m = M.MetaModel([b"/svc/M"])
    req = [(b":method", b"POST"), (b":scheme", b"http"), (b":path", b"/svc/M"), (b"content-type", b"application/grpc"), (b"te", b"trailers"),
           (b"grpc-timeout", b"2562048H"), (b"x-a", b"b")]
    recs = m.read(*pack([(7, 0, req), (9, 1, [(b"grpc-status", b"14")])]), 2, 1)[0]
    view = h2dev.CallMetadata.records(b"".join(M.record_bytes(r) for r in recs))
    assert h2dev.CALL_META.itemsize == 48 and view.dtype == h2dev.CALL_META and len(view) == 2
    assert [tuple(int(x) for x in row) for row in view] == [tuple(r) for r in recs]
    assert list(view["stream"]) == [7, 9] and list(view["method"]) == [0, M.NONE] and list(view["grpc_status"]) == [M.NONE, 14]
    assert (int(view["timeout_hi"][0]) << 32 | int(view["timeout_lo"][0])) == 2**63 - 1 and int(view["ncustom"][0]) == 1
    assert (h2dev.CallMetadata.REQUEST, h2dev.CallMetadata.BAD_GRPC_STATUS, h2dev.CallMetadata.HAS_MESSAGE) == (M.REQUEST, M.BAD_GRPC_STATUS,
                                                                                                               M.HAS_MESSAGE)


def test_caps_and_bad_input_in_the_model():
    m = M.MetaModel([b"/svc/M"])
    req = [(b":method", b"POST"), (b":scheme", b"http"), (b":path", b"/svc/N"), (b"content-type", b"application/grpc"), (b"te", b"trailers")]
    blocks, fields, arena = pack([(1, 0, req), (3, 0, req)])
    assert m.read(blocks, fields, arena, 1, 2)[2:] == ((2, 2, 0, 0, 2, 0, 0, 1), "capacity")
    assert m.read(blocks, fields, arena, 2, 1)[2:] == ((2, 2, 0, 0, 2, 0, 0, 1), "capacity") and m.stats["calls"] == 0
    assert m.read(blocks, fields, arena, 2, 2)[2:] == ((2, 2, 0, 0, 2, 0, 0, 0), None) and m.stats["rejections"] == 2
    bad = [blocks[0], (0,) + blocks[1][1:]]
    assert m.read(bad, fields, arena, 2, 2)[2:] == ((0, 0, 0, 0, 0, 0, M.BAD_INPUT | M.ERR_STREAM << 8 | 1 << 32, 0), "invalid")
