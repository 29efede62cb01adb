"""The harness of the many-link header encoder's tests (tests/test_zz_gpu_h2_links_hpenc.py): one h2dev.encode_batch call
over harnesses of tests/h2_hpenc_lib.py (HE: a device encoder with the HpencModel beside it), every listed link compared
with its own model as HE.encode compares a single call: the WHOLE wire arena and block-wire table (what is not written
keeps its fill), the result tuple, the table dump and the counters.  pytest rewrites no `assert` in a helper module:
every check goes through `same`."""
import copy

from tests.h2_hpenc_lib import HE, SENTINEL, Input, Wire, bw_bytes  # noqa: F401  (HE, Input: for the tests)
from tests.h2_hpenc_model import pack


def table_words(data, n):
    """n rows of four 32-bit words out of a block or field table read from the device"""
    return [tuple(int.from_bytes(data[16 * i + 4 * j:16 * i + 4 * j + 4], "little") for j in range(4)) for i in range(n)]


def item_of(h, inp_args):
    """an item of h2dev.encode_batch: the harness's encoder, the six input arguments and its wire targets (h.out)"""
    return (h.enc,) + tuple(inp_args) + h.out.args()


def prepare(hs, order, lists=None, raw=None, caps=None, device=None):
    """every listed link's model stepped and its SENTINEL-filled targets made (hs[i].out), its input uploaded unless it
    stands on the device already -> (the items of the call in order, {i: what the model says: (wire, block-wire table,
    result, error)}).  lists: {i: [(stream, flags, [(name, value[, hint])])]}, or raw: {i: (blocks, fields, arena)} as
    they are; caps: {i: (wire cap or None, block-wire cap or None)} where a link's differ from what its call needs and 8
    bytes, one entry more; device: {i: (the six input arguments, (blocks, fields, arena) as the tables there hold them)}"""
    lists, raw, caps, device = lists or {}, raw or {}, caps or {}, device or {}
    items, exp = [], {}
    for i in order:
        h = hs[i]
        args = None
        if i in device:
            args, (blocks, fields, arena) = device[i]
        else:
            blocks, fields, arena = raw[i] if i in raw else pack(lists[i])
        wire_cap, bw_cap = caps.get(i, (None, None))
        if wire_cap is None or bw_cap is None:
            need = copy.deepcopy(h.model).encode(blocks, fields, arena, 1 << 40, 1 << 40)[2]
            wire_cap = need[2] + 8 if wire_cap is None else wire_cap
            bw_cap = need[0] + 1 if bw_cap is None else bw_cap
        exp[i] = h.model.encode(blocks, fields, arena, wire_cap, bw_cap)
        if args is None:
            h.inp = Input(h.g, blocks, fields, arena)
            args = h.inp.args()
        h.out = Wire(h.g, max(1, wire_cap), max(1, bw_cap))
        items.append(item_of(h, args))
    return items, exp


def compare(hs, order, exp, count, got):
    """what an encode_batch call left against what the models say -> {i: (wire bytes, block-wire table, result)}"""
    from tests.h2_device_lib import same
    same(count, sum(1 for i in order if exp[i][3] is None), "encode_batch: the items on the wire")
    out = {}
    for i, res_d in zip(order, got):
        wire, bw, res, _err = exp[i]
        what = "link %d: " % i
        print("%sencode: %r -> %r" % (what, res, res_d))
        same(res_d, res, what + "result")
        same(hs[i].enc.last_result, res, what + ".last_result")
        w, b = hs[i].out.wire.read(), hs[i].out.bw.read()
        same(w, wire + bytes([SENTINEL]) * (len(w) - len(wire)), what + "the whole wire arena")
        same(b, bw_bytes(bw) + bytes([SENTINEL]) * (len(b) - 16 * len(bw)), what + "the whole block-wire table")
        hs[i].check()
        out[i] = (wire, bw, res)
    return out


def encode_batch(hs, order, **kw):
    """encode on the links hs[i], i in order, in one batch call on the device and in each link's model, compare
    everything -> (the call's return value, {i: (wire bytes, block-wire table, result)}); the arguments: prepare's"""
    from grpc_rdma_amd import h2dev
    items, exp = prepare(hs, order, **kw)
    count, got = h2dev.encode_batch(items)
    return count, compare(hs, order, exp, count, got)


def unchanged(hs, what):
    """every harness's table and counters are its model's still, and its wire targets hold nothing but their fill"""
    from tests.h2_device_lib import same
    for k, h in enumerate(hs):
        h.check()
        for buf in (h.out.wire, h.out.bw):
            data = buf.read()
            same(data, bytes([SENTINEL]) * len(data), "%s: nothing written on link %d" % (what, k))
