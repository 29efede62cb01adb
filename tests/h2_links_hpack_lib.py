"""The harness of the many-link header decoder's tests (tests/test_zz_gpu_h2_links_hpack.py): one h2dev.decode_batch call over harnesses of tests/h2_hpack_lib.py (HH: a device parser with its header decoder, the
oracle's parser and the HpackModel beside them), every listed link compared with its own model as HH.decode compares a
single call.  pytest rewrites no `assert` in a helper module: every check goes through `same`."""
from tests.h2_hpack_lib import HH, SENTINEL, Targets, _words  # noqa: F401  (HH: for the tests)


def _step(hs, order, caps, lost):
    """every listed link's model stepped over its last deframing and SENTINEL-filled targets -> per link (targets, what
    the model says: blocks, fields, strings, result)"""
    caps = caps or {}
    exp = {}
    for i in order:
        h = hs[i]
        c = caps.get(i, h.caps)
        h.target = Targets(h.g, *c)
        err_o, ev_o = h.last
        blocks, fields, strings, res, _rc = h.model.decode(ev_o, h.last_slices, err_o, c, skipped=h.skipped, lost=h.lost or i in lost)
        if res[7] != 1:
            h.skipped = h.lost = False
        exp[i] = (blocks, fields, strings, res)
    return exp


def decode_batch_raw(hs, order, caps=None):
    """grdma_h2_hpack_decode_batch itself, into fresh targets; no model is stepped -> (its return value, the result
    tuples as the call left them)"""
    import ctypes as C
    from grpc_rdma_amd import h2dev
    arr = (h2dev.H2HpackItem * len(order))()
    for k, i in enumerate(order):
        h = hs[i]
        h.target = Targets(h.g, *(caps or {}).get(i, h.caps))
        arr[k].hpack = h.dec.h
        (arr[k].d_blocks, arr[k].blocks_cap, arr[k].d_fields, arr[k].fields_cap, arr[k].d_strings, arr[k].strings_cap) = h.target.args()
    out = (C.c_uint64 * (8 * len(order)))()
    rc = h2dev.load().grdma_h2_hpack_decode_batch(arr, len(order), out)
    return rc, [tuple(int(x) for x in out[8 * k:8 * k + 8]) for k in range(len(order))]


def decode_batch(hs, order, caps=None, lost=()):
    """decode the last deframing of the links hs[i], i in order, in one batch call on the device and in each link's
    model, compare everything -> {i: (blocks, result)}: blocks as [(stream, flags, [(name, value, representation)])].
    caps: {i: (blocks, fields, strings)} where a link's differ from its harness's; lost: links whose event list
    overflowed"""
    from grpc_rdma_amd import h2dev
    from tests.h2_device_lib import same
    exp = _step(hs, order, caps, lost)
    count, got = h2dev.decode_batch([(hs[i].dec,) + hs[i].target.args() for i in order])
    same(count, sum(1 for i in order if exp[i][3][7] == 0), "decode_batch: the items without overflow")
    out = {}
    for i, res_d in zip(order, got):
        blocks, fields, strings, res = exp[i]
        what = "link %d: " % i
        print("%sdecode: %r -> %r" % (what, res, res_d))
        same(res_d, res, what + "result")
        same(hs[i].dec.last_result, res, what + ".last_result")
        b, f, s = hs[i].target.read()
        same(b, _words(blocks) + bytes([SENTINEL]) * (len(b) - 16 * len(blocks)), what + "the whole block table")
        same(f, _words(fields) + bytes([SENTINEL]) * (len(f) - 16 * len(fields)), what + "the whole field table")
        same(s, strings + bytes([SENTINEL]) * (len(s) - len(strings)), what + "the whole string arena")
        hs[i].check()
        out[i] = ([(stream, flags, [(strings[no:no + (nl & 0xffffff)], strings[vo:vo + vl], nl >> 24) for no, vo, nl, vl in fields[first:first + n]])
                   for stream, first, n, flags in blocks], res)
    return out
