"""What the metadata reader's tests share (tests/test_zz_gpu_h2_meta.py, tests/test_h2_meta_model.py,
tools/h2_meta_probe.py): the harness of the device tests -- a device reader (h2dev.CallMetadata) and the model of
tests/h2_meta_model.py beside it, every call compared whole -- the colliding pair of the method table's hash, and the
builders of the cases' header lists.  pytest rewrites no `assert` in a helper module: every check goes through `same`."""
from tests.h2_hpenc_lib import ERR2, ERR5, SENTINEL, Input
from tests.h2_hpenc_model import pack
from tests.h2_meta_model import ENCODINGS, MetaModel, accept_bits, record_bytes

# Found once by a birthday search over "/svc/" and eight random characters (FNV-1a, 32 bits);
# tests/test_h2_meta_model.py::test_the_colliding_paths_collide holds them.
PATH_COLLISION = (b"/svc/a8iz9pgm", b"/svc/g5snxjzz")
PATH = b"/svc/M"


def _words(rows):
    return b"".join(int(w).to_bytes(4, "little") for r in rows for w in r)


class Out:
    """a record table and a rejection list filled with SENTINEL, with room behind the caps"""

    def __init__(self, g, meta_cap, reject_cap):
        self.caps = (meta_cap, reject_cap)
        self.meta = g.DeviceBuffer(data=bytes([SENTINEL]) * (48 * (meta_cap + 2)))
        self.reject = g.DeviceBuffer(data=bytes([SENTINEL]) * (16 * (reject_cap + 4)))

    def args(self):
        return (self.meta.ptr, self.caps[0], self.reject.ptr, self.caps[1])


class MH:
    def __init__(self, g, methods=(PATH,), accept=("identity",)):
        from grpc_rdma_amd import h2dev
        self.g = g
        self.dev = h2dev.CallMetadata(methods=methods, accept=accept)
        self.model = MetaModel(methods, accept_bits(accept))
        self.check()
        from tests.h2_device_lib import device_bytes, same
        fp, nf, sp, nb = self.dev.reject_tables()
        same(device_bytes(g, fp, 16 * nf), _words(self.model.reject_fields), "the constant field table")
        same(device_bytes(g, sp, nb), self.model.reject_arena, "the constant string arena")

    def read(self, lists=None, raw=None, meta_cap=None, reject_cap=None, device=None):
        """one call on the device and in the model, everything compared -> (call records, rejection blocks, result
        tuple).  lists: [(stream, flags, [(name, value)])], or raw: (blocks, fields, arena) as they are; the caps default
        to what the call needs and one more.  device: the six input arguments where the three tables stand in device
        memory already (raw: what they hold)"""
        import pytest
        from tests.h2_device_lib import same
        blocks, fields, arena = pack(lists) if raw is None else raw
        if meta_cap is None or reject_cap is None:
            import copy
            need = copy.deepcopy(self.model).read(blocks, fields, arena, 1 << 40, 1 << 40)[2]
            meta_cap = need[0] + 1 if meta_cap is None else meta_cap
            reject_cap = need[4] + 1 if reject_cap is None else reject_cap
        recs, rej, res, err = self.model.read(blocks, fields, arena, meta_cap, reject_cap)
        inp, out = None if device else Input(self.g, blocks, fields, arena), Out(self.g, max(1, meta_cap), max(1, reject_cap))
        args = tuple(device or inp.args()) + out.args()
        if err:
            with pytest.raises(self.g.GrdmaError, match=ERR5 if err == "capacity" else ERR2):
                self.dev.read(*args)
            got = self.dev.last_result
        else:
            n, got = self.dev.read(*args)
            same(n, res[4], "read: the number of rejection blocks")
        print("read: %r -> %r" % (res, got))
        same(got, res, "read: result")
        m, r = out.meta.read(), out.reject.read()
        want = b"".join(record_bytes(x) for x in recs)
        if m != want + bytes([SENTINEL]) * (len(m) - len(want)):  # (say which record, then fail on the bytes)
            for k, x in enumerate(recs):
                same(tuple(int.from_bytes(m[48 * k + 4 * j:48 * k + 4 * j + 4], "little") for j in range(12)), x, "read: call record %d" % k)
        same(m, want + bytes([SENTINEL]) * (len(m) - len(want)), "read: the whole record table")
        same(r, _words(rej) + bytes([SENTINEL]) * (len(r) - 16 * len(rej)), "read: the whole rejection list")
        self.check()
        self.last_out = out
        return recs, rej, res

    def check(self):
        from tests.h2_device_lib import same
        st = self.dev.stats()
        same({k: st[k] for k in self.model.stats}, self.model.stats, "counters (all: %r)" % (st,))
        fp, nf, sp, nb = self.dev.reject_tables()
        same((nf, nb), (len(self.model.reject_fields), len(self.model.reject_arena)), "the constant tables' sizes")

    def close(self):
        self.dev.close()


# ---- a record's parts -----------------------------------------------------------------------------------------------------
def kind(rec):
    return rec[1] & 0xff


def verdict(rec):
    return rec[1] >> 8 & 0xff


def encoding(rec):
    return rec[1] >> 16 & 0xff


def flags(rec):
    return rec[1] >> 24


def timeout(rec):
    return rec[5] | rec[6] << 32


# ---- header lists for the cases ---------------------------------------------------------------------------------------------
def request(path=PATH, drop=(), **over):
    """a good request's header list; drop: names left out; over: name=value with '_' for '-' and a leading 'p_' for ':'
    (p_method=b"GET", grpc_timeout=b"1S"); a name that is new goes behind the others"""
    hs = [(b":method", b"POST"), (b":scheme", b"http"), (b":path", path), (b":authority", b"host"), (b"content-type", b"application/grpc"),
          (b"te", b"trailers")]
    names = {(":" + k[2:] if k.startswith("p_") else k).replace("_", "-").encode(): v for k, v in over.items()}
    hs = [(n, names.pop(n, v)) for n, v in hs if n not in drop]
    return hs + list(names.items())


def response(status=b"200", content_type=b"application/grpc", extra=()):
    return [(b":status", status)] + ([(b"content-type", content_type)] if content_type is not None else []) + list(extra)


def trailers(status=b"0", extra=()):
    return ([(b"grpc-status", status)] if status is not None else []) + list(extra)


def customs(n, stem=b"k"):
    """n regular fields no key knows"""
    return [(b"x-%s%04d" % (stem, i), b"v%04d" % i) for i in range(n)]


assert ENCODINGS == (b"identity", b"gzip", b"deflate")
