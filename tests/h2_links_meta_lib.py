"""The harness of the many-link metadata reader's tests (tests/test_zz_gpu_h2_links_meta.py): one CallMetadata.read_batch
call over ONE harness of tests/h2_meta_lib.py (MH: a device reader with the MetaModel beside it).  The reference of a
batch is that one model's `read`, called per item in item order -- so its counters sum over the items read as the
device's must -- with `calls` set back to ONE call where more than one item was read.  Every item is compared whole: the
WHOLE record table and the WHOLE rejection list (what is not written keeps its fill), the result tuple and, behind the
call, the reader's counters.  pytest rewrites no `assert` in a helper module: every check goes through `same`."""
import copy

from tests.h2_hpenc_lib import SENTINEL, Input  # noqa: F401  (Input: for the tests)
from tests.h2_hpenc_model import pack
from tests.h2_meta_lib import MH, Out, _words  # noqa: F401  (MH: for the tests)
from tests.h2_meta_model import record_bytes

# grdma_h2_meta_item's members in order: the ten arguments of CallMetadata.read, every one a 64-bit word
ITEM_FIELDS = ("d_blocks", "nblocks", "d_fields", "nfields", "d_strings", "strings_bytes", "d_meta", "meta_cap", "d_reject", "reject_cap")


def item_dtype():
    """the numpy structured dtype of grdma_h2_meta_item: a row of the (n, 10) array CallMetadata.read_batch fills"""
    import numpy as np
    return np.dtype([(name, "<u8") for name in ITEM_FIELDS])


class Link:
    """what one item of a call leaves behind: its input on the device (None where it was shared or stood there), its
    SENTINEL-filled targets, and what the model says: (call records, rejection blocks, result, error)"""

    def __init__(self, inp, out, exp):
        self.inp, self.out, self.exp = inp, out, exp


def model_batch(model, tables, caps):
    """the model of one batch: `read` per item in item order, then ONE call where items were read -> [(call records,
    rejection blocks, result, error)]"""
    exp = [model.read(blocks, fields, arena, mc, rc) for (blocks, fields, arena), (mc, rc) in zip(tables, caps)]
    read = sum(1 for e in exp if e[3] is None)
    if read > 1:
        model.stats["calls"] -= read - 1
    return exp


def prepare(h, order, lists=None, raw=None, caps=None, device=None):
    """the model stepped over the items in order and every item's SENTINEL-filled targets made, its input uploaded unless
    it stands on the device already -> (the items of the call in order, {i: Link}).  lists: {i: [(stream, flags, [(name,
    value)])]}, or raw: {i: (blocks, fields, arena)} as they are; caps: {i: (record cap or None, rejection cap or None)}
    where an item's differ from what its call needs and one more; device: {i: (the six input arguments, (blocks, fields,
    arena) as the tables there hold them)} -- many items may name one input"""
    lists, raw, caps, device = lists or {}, raw or {}, caps or {}, device or {}
    tables, args, inps, use = [], [], [], []
    for i in order:
        if i in device:
            a, t = device[i]
            inp = None
        else:
            t = raw[i] if i in raw else pack(lists[i])
            inp = Input(h.g, *t)
            a = inp.args()
        meta_cap, reject_cap = caps.get(i, (None, None))
        if meta_cap is None or reject_cap is None:
            need = copy.deepcopy(h.model).read(t[0], t[1], t[2], 1 << 40, 1 << 40)[2]
            meta_cap = need[0] + 1 if meta_cap is None else meta_cap
            reject_cap = need[4] + 1 if reject_cap is None else reject_cap
        tables.append(t)
        args.append(tuple(a))
        inps.append(inp)
        use.append((meta_cap, reject_cap))
    exp = model_batch(h.model, tables, use)
    items, links = [], {}
    for i, a, inp, (meta_cap, reject_cap), e in zip(order, args, inps, use, exp):
        out = Out(h.g, max(1, meta_cap), max(1, reject_cap))
        links[i] = Link(inp, out, e)
        items.append(a + out.args())
    return items, links


def compare(h, order, links, count, got, counters=True):
    """what a read_batch call left against what the model says -> {i: (call records, rejection blocks, result)};
    counters False: the reader is closed by now"""
    from tests.h2_device_lib import same
    same(count, sum(1 for i in order if links[i].exp[3] is None), "read_batch: the items read")
    same(h.dev.last_results, got, "read_batch: .last_results")
    out = {}
    for i, res_d in zip(order, got):
        recs, rej, res, _err = links[i].exp
        what = "item %d: " % i
        print("%sread: %r -> %r" % (what, res, res_d))
        same(res_d, res, what + "result")
        m, r = links[i].out.meta.read(), links[i].out.reject.read()
        want = b"".join(record_bytes(x) for x in recs)
        if m != want + bytes([SENTINEL]) * (len(m) - len(want)):  # (say which record, then fail on the bytes)
            for k, x in enumerate(recs):
                same(tuple(int.from_bytes(m[48 * k + 4 * j:48 * k + 4 * j + 4], "little") for j in range(12)), x, what + "call record %d" % k)
        same(m, want + bytes([SENTINEL]) * (len(m) - len(want)), what + "the whole record table")
        same(r, _words(rej) + bytes([SENTINEL]) * (len(r) - 16 * len(rej)), what + "the whole rejection list")
        out[i] = (recs, rej, res)
    if counters:
        h.check()
    return out


def read_batch(h, order, **kw):
    """read the items i in order in one batch call on the device and in the model, compare everything -> (the call's
    return value, {i: (call records, rejection blocks, result)}, {i: Link}); the arguments: prepare's"""
    items, links = prepare(h, order, **kw)
    count, got = h.dev.read_batch(items)
    return count, compare(h, order, links, count, got), links


def unchanged(h, links, what):
    """the reader's counters are its model's still, and every item's targets hold nothing but their fill"""
    from tests.h2_device_lib import same
    h.check()
    for i, ln in links.items():
        for buf in (ln.out.meta, ln.out.reject):
            data = buf.read()
            same(data, bytes([SENTINEL]) * len(data), "%s: nothing written for item %d" % (what, i))
