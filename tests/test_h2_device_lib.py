"""The inputs of the HTTP/2 device tests, pinned with no device: the arena packer in every layout and the seeded wire
generators of tests/h2_device_lib.py at seeds the tests use.  The GPU files compare device output with values derived
from these bytes, so a helper that drifts would move every expected value with it, unseen.

Every literal below was produced by the spellings these helpers replaced, run at the commit before the helpers were
gathered (_slice_table, _table, Transport.item, the two gpu_events and pack for the packer; the generators from the
test files they lived in) -- never by the code under test.  A digest is the first 16 hex digits of sha256 over the
parts, each followed by "|"; a part that is not bytes goes in as its repr."""
import hashlib
import random

import pytest

from tests import h2_device_lib as lib
from tests.h2_device_lib import PADDED, STEPPED, UNPADDED, pack_slices


def dg(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, (bytes, bytearray)) else repr(p).encode())
        h.update(b"|")
    return h.hexdigest()[:16]


LISTS = {
    "small": [b"a" * 5, b"", b"b" * 16, b"c" * 33],
    "two": [bytes(range(40)), b"x"],
    "twenty": [bytes([k]) * ((7 * k) % 23) for k in range(20)],
}
# (layout, list, with random.Random(5)) -> (digest of the arena, digest of the table, the generator's next random())
PACK = {
    (PADDED, "small", False): ("6798685127d48cc2", "512a1fcac0af31e8", None),
    (PADDED, "small", True): ("99f9b770b63ec3a2", "2164328cf25743ae", 0.7951935655656966),
    (PADDED, "twenty", False): ("b7fcbe6397272426", "f42f72c56787b0cf", None),
    (PADDED, "twenty", True): ("6da2562262b645d5", "4d283e70569b8040", 0.11320596465314436),
    (PADDED, "two", False): ("4802aee599492eee", "57c59448e957e6e5", None),
    (PADDED, "two", True): ("52049b84ab1ee936", "aac08c17ae4702f7", 0.7417869892607294),
    (STEPPED, "small", False): ("2d00f91a9dfa4c58", "0351aeff8708464b", None),
    (STEPPED, "twenty", False): ("02a802461b37ec85", "4d12358d0c751689", None),
    (STEPPED, "two", False): ("5396dfa4b30ff5f1", "b7e471674be7d856", None),
    (UNPADDED, "small", False): ("7ab44e3fd28e98a2", "512a1fcac0af31e8", None),
    (UNPADDED, "small", True): ("872a3b2ce43d6315", "cc0a04e8ff8aaa89", 0.7951935655656966),
    (UNPADDED, "twenty", False): ("f29f801bfea4563a", "f42f72c56787b0cf", None),
    (UNPADDED, "twenty", True): ("014394f4d111aedc", "9a61953c0b0c886c", 0.11320596465314436),
    (UNPADDED, "two", False): ("953b2a10e2bbc39b", "57c59448e957e6e5", None),
    (UNPADDED, "two", True): ("59b8a98331a0c8a5", "7821a8c8ae645c27", 0.7417869892607294),
}


@pytest.mark.parametrize("layout,name,seeded", sorted(PACK))
def test_pack_slices_lays_out_what_the_replaced_spellings_did(layout, name, seeded):
    rng = random.Random(5) if seeded else None
    data, table = pack_slices(LISTS[name], layout, rng)
    assert (dg(data), dg(table), rng.random() if rng else None) == PACK[(layout, name, seeded)]
    # what every layout promises: the table names the slices, 64 zero bytes (at least) behind the last one
    assert [data[o:o + n] for o, n in table] == LISTS[name] and data[-64:] == bytes(64)
    assert table[-1][0] + table[-1][1] + 64 <= len(data)


def test_layouts_without_a_generator_agree_on_the_table():
    for sl in LISTS.values():
        assert pack_slices(sl, PADDED)[1] == pack_slices(sl, UNPADDED)[1]
        assert all(o % 16 == 0 for o, _ in pack_slices(sl, PADDED)[1])


BIG_IDS = (0x01020305, 0x7FFFFFFF, 0x7F000001, 0x00FF0001)


def test_eight_streams():
    exp = {(0, 4): (298766, "72fec85707a753f8", "82cc09c021a58fc3"), (1, 4): (390843, "63c1ed1bb2dd710a", "8905429d630d6a98"),
           (2, 4): (141577, "bdcd3ed9b2b075b2", "24b54c41376dcc26"), (41, 2): (252645, "4b4c7ce586d57ae4", "9df3327d7ccb859a"),
           (42, 2): (132412, "ef5b2f1639427625", "d53115d145da5183"), (77, 2): (209510, "96ce7187a49078c2", "82299a1bcd5821a1")}
    for (seed, nmsg), want in exp.items():
        wire, parts = lib._eight_streams(seed, nmsg=nmsg)
        assert (len(wire), dg(wire), dg([len(p) for p in parts])) == want, (seed, nmsg)
        assert b"".join(parts) == wire


def test_batch_and_batches():
    assert dg(lib.BATCHES) == "aecce9d423b1fd5e"
    exp = [(([3, 70000, 16379, 16380], 16384, 4), ("10f170fec0760c2d", "8dddf7364d742848", "51b10adb02c4ccab")),
           (([100, 0, 17], 3, 3), ("e61be4905c961f30", "545e94bf49c5bf2e", "a21231c4c174ac07")),
           (([20, 0, 21, 22, 0, 0, 23, 24], 5, 8), ("416938a82c5c2558", "9e5a3b5c5b5793d2", "bcd7cc4fb523e1c0")),
           (([20, 0, 21, 22, 0, 0, 23, 24], 5, 9), ("74e22bd26572584e", "7e7dd5ce3a33c2a4", "bcd7cc4fb523e1c0")),
           (([3, 70000, 16379, 0, 5], 16384, 4), ("d89789542de4d4b0", "116806cd0229ffa1", "97f7b213db8afd3b")),
           (([1000, 0, 70000], 16384, 2), ("65b58fd45e58781d", "8ae4400c5dffd36d", "85b9c05eabeec190"))]
    for args, want in exp:
        bodies, wire, slices = lib._batch(*args)
        assert (dg(*bodies), dg(wire), dg([len(x) for x in slices])) == want, args
        assert b"".join(slices) == wire and [len(b) for b in bodies] == args[0]


def test_client_stream_and_the_cuts():
    exp = {(32, (1, 3, 5), 9): (45546, "c3872761b99d781c"), (33, (7,), 6): (15444, "a8136f93642c66a8"),
           (3, (1, 3), 7): (90195, "adbaf34ebbd9d75b"), (21, (1,), 4): (20106, "16935ef7c22608dc"),
           (22, (1, 3), 5): (25141, "ef2ef9899e561bc3")}
    for (seed, sids, n), want in exp.items():
        w = lib._client_stream(seed, list(sids), n)
        assert (len(w), dg(w)) == want, (seed, sids, n)
    data = bytes(range(200))
    assert dg(*lib.cut_points(data, random.Random(9), 5)) == "824810b67588ee12"
    assert dg(*lib.cut_points(data, random.Random(9), 500)) == "9ca1b516734454ae"
    assert dg(*lib.cut_mean(data, random.Random(4))) == "1aaf63f440b4178f"
    assert dg(*lib.cut_mean(data, random.Random(4), 5)) == "577a287bf76a78ff"
    for pieces in (lib.cut_points(data, random.Random(9), 5), lib.cut_mean(data, random.Random(4), 5)):
        assert b"".join(pieces) == data and all(pieces)


def test_flow_wires_and_link_tables():
    assert dg(lib.FLOW_SIZES) == "fa111542cdb9d426" and dg(lib.TABLES) == "96f4f72ddc0d1f2a"
    assert dg(*lib._interleaved(0, (1, 3, 5), lib.FLOW_SIZES)) == "672996a41f4880b8"
    assert dg(*lib._interleaved(1, BIG_IDS, lib.FLOW_SIZES[:6])) == "022b0e9eb9655f87"
    assert dg(*lib._server_open((1, 3, 5))) == "c26552eecbb7a301"


def test_sender_and_receiver_slices():
    for args, kw, want in ((([100000] * 3,), {}, (42, "c39069285a745073")),
                           (([5, 100000, 16379],), dict(seed=9), (18, "fe85dca356d344bc")),
                           (([3072] * 3,), dict(sid=33, max_frame=1024), (24, "11e0833b4970b596"))):
        sl = lib.fast_sender_slices(*args, **kw)
        assert (len(sl), dg(*sl)) == want, (args, kw)
    tx = lib.sender_slices([7, 40000, 16379], sid=3, seed=2)
    assert (len(tx), dg(*tx)) == (10, "0bd93b9048fce896")
    rx = lib.receiver_slices(tx)
    assert (len(rx), dg(*rx)) == (8, "87e6ccbec32488f0") and b"".join(rx) == b"".join(tx)
    # fast_sender_slices is sender_slices with numpy payloads, but for END_STREAM
    assert lib.fast_sender_slices([7, 40000, 16379], sid=3, seed=2) == lib.sender_slices([7, 40000, 16379], sid=3, end_stream=False, seed=2)


def test_same_names_the_first_difference():
    lib.same([1, 2, 3], [1, 2, 3])
    with pytest.raises(AssertionError, match=r"events: item 1 of 3 / 2: device \[\(9, 9\)\], expected \[\(2, 2\)\]"):
        lib.same([(1, 1), (9, 9), (3, 3)], [(1, 1), (2, 2)], "events")
    with pytest.raises(AssertionError, match=r"wire: item 2 of 4 / 4: device 0304, expected ff04"):
        lib.same(b"\x01\x02\x03\x04", b"\x01\x02\xff\x04", "wire")
    with pytest.raises(AssertionError, match=r"live: device 3, expected 4"):
        lib.same(3, 4, "live")
