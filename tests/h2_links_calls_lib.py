"""The harness of the many-link call table's tests (tests/test_zz_gpu_h2_links_calls.py): one h2dev.calls_step_batch call
over n harnesses of tests/h2_calls_lib.py (CH: a device table with the CallsModel of tests/h2_calls_model.py beside it).
The reference of a batch is every item's own model, stepped independently, in item order.  Every item is compared whole:
the WHOLE dispatch table, the segment words and the WHOLE done list (what is not written keeps its SENTINEL fill), the
result tuple and, behind the call, the table's dump and counters.  pytest rewrites no `assert` in a helper module: every
check goes through `same`."""
import copy
import struct

from tests.h2_calls_lib import BIG, CH, Out, Tables, filled  # noqa: F401  (CH, Out, Tables: for the tests)
from tests.h2_calls_model import dispatch_bytes, done_bytes

# grdma_h2_calls_item's members in order: the table and the thirteen arguments of CallTable.step, every one a 64-bit word
ITEM_FIELDS = ("calls", "d_blocks", "d_meta", "nblocks", "d_msgs", "nmsgs", "d_events", "nevents", "now_ns", "d_dispatch", "dispatch_cap",
               "d_segments", "d_done", "done_cap")


def item_dtype():
    """the numpy structured dtype of grdma_h2_calls_item: a row of the (n, 14) array h2dev.calls_step_batch fills"""
    import numpy as np
    return np.dtype([(name, "<u8") for name in ITEM_FIELDS])


class Link:
    """what one item of a call leaves behind: its input on the device (None where it was shared or stood there), its
    SENTINEL-filled targets, and what its model says: (dispatch records, segment words, done records, result, error)"""

    def __init__(self, inp, out, exp):
        self.inp, self.out, self.exp = inp, out, exp


def prepare(hs, order, steps=None, caps=None, device=None):
    """every item's model stepped, in item order, its SENTINEL-filled targets made and its input uploaded unless it stands
    on the device already -> (the items of the call in order, {i: Link}).  steps: {i: dict(reqs=, msgs=, events=, now=)}
    (CH.step's, all optional; an i without entry is an empty step at now 0); caps: {i: (dispatch cap or None, done cap or
    None)} where an item's differ from what its step needs and one more; device: {i: the seven input arguments} where the
    tables stand in device memory already (steps[i]: what they hold) -- many items may name one input"""
    steps, caps, device = steps or {}, caps or {}, device or {}
    items, links = [], {}
    for i in order:
        h, s = hs[i], steps.get(i, {})
        reqs, msgs, events, now = list(s.get("reqs", ())), list(s.get("msgs", ())), list(s.get("events", ())), s.get("now", 0)
        blocks, meta = [r[0] for r in reqs], [r[1] for r in reqs]
        dispatch_cap, done_cap = caps.get(i, (None, None))
        if dispatch_cap is None or done_cap is None:
            need = copy.deepcopy(h.model).step(blocks, meta, msgs, events, now, BIG, BIG)[3]
            dispatch_cap = len(msgs) + 1 if dispatch_cap is None else dispatch_cap
            done_cap = need[3] + 1 if done_cap is None else done_cap
        exp = h.model.step(blocks, meta, msgs, events, now, dispatch_cap, done_cap)
        inp = None if i in device else Tables(h.g, blocks, meta, msgs, events)
        out = Out(h.g, max(1, dispatch_cap), max(1, done_cap), h.nmethods)
        links[i] = Link(inp, out, exp)
        items.append((h.dev,) + tuple(device[i] if i in device else inp.args()) + (now,) + out.args())
    return items, links


def compare_targets(what, ln):
    """an item's three targets against what its model says, whole"""
    from tests.h2_device_lib import same
    disp, segs, done, _res, _err = ln.exp
    d, s, f = ln.out.dispatch.read(), ln.out.segments.read(), ln.out.done.read()
    for k, x in enumerate(disp):  # (say which record, then fail on the bytes)
        if d[48 * k:48 * k + 48] != dispatch_bytes(x):
            same(struct.unpack("<QQQIIIIII", d[48 * k:48 * k + 48]), x, what + "dispatch record %d" % k)
    same(d, filled(b"".join(dispatch_bytes(x) for x in disp), len(d)), what + "the whole dispatch table")
    same(s, filled(b"" if segs is None else struct.pack("<%dI" % len(segs), *segs), len(s)), what + "the segment words")
    for k, x in enumerate(done):
        if f[32 * k:32 * k + 32] != done_bytes(x):
            same(struct.unpack("<QQIIII", f[32 * k:32 * k + 32]), x, what + "done record %d" % k)
    same(f, filled(b"".join(done_bytes(x) for x in done), len(f)), what + "the whole done list")


def compare(hs, order, links, count, got, tables=True):
    """what a calls_step_batch call left against what the models say -> {i: (dispatch records, segment words, done
    records, result)}; tables False: the tables are closed by now"""
    from tests.h2_device_lib import same
    same(count, sum(1 for i in order if links[i].exp[4] is None), "calls_step_batch: the items that committed")
    out = {}
    for i, res_d in zip(order, got):
        disp, segs, done, res, _err = links[i].exp
        what = "item %d: " % i
        print("%sstep: %r -> %r" % (what, res, res_d))
        same(res_d, res, what + "result")
        same(hs[i].dev.last_result, res, what + ".last_result")
        compare_targets(what, links[i])
        if tables:
            hs[i].check()
        out[i] = (disp, segs, done, res)
    return out


def step_batch(hs, order, **kw):
    """step the tables i in order in one batch call on the device and in their models, compare everything -> (the call's
    return value, {i: (dispatch records, segment words, done records, result)}, {i: Link}); the arguments: prepare's"""
    from grpc_rdma_amd import h2dev
    items, links = prepare(hs, order, **kw)
    count, got = h2dev.calls_step_batch(items)
    return count, compare(hs, order, links, count, got), links


def unchanged(hs, links, what):
    """every table's dump and counters are its model's still, and every item's targets hold nothing but their fill"""
    from tests.h2_device_lib import same
    from tests.h2_hpenc_lib import SENTINEL
    for h in hs:
        h.check()
    for i, ln in links.items():
        for buf in (ln.out.dispatch, ln.out.segments, ln.out.done):
            data = buf.read()
            same(data, bytes([SENTINEL]) * len(data), "%s: nothing written for item %d" % (what, i))
