"""What the header encoder's tests share (tests/test_zz_gpu_h2_hpenc.py, tests/test_h2_hpenc_model.py,
tools/h2_hpenc_probe.py): the harness of the device tests -- a device encoder (h2dev.HeaderEncoder) and the model of
tests/h2_hpenc_model.py beside it, every call compared whole -- the colliding pairs of the hash, and the builders of the
cases' header lists.  pytest rewrites no `assert` in a helper module: every check goes through `same`."""
from tests.h2_hpack_model import HUFFMAN
from tests.h2_hpenc_model import CHUNK, HpencModel, pack

SENTINEL = 0xA5
ERR5, ERR2 = "error 5", "error 2"  # -GRDMA_ERR_CAPACITY, -GRDMA_ERR_INVALID

# Found once by a birthday search over random lower-case strings (FNV-1a, 32 bits: some hundred thousand suffice);
# tests/test_h2_hpenc_model.py::test_the_hash_is_fnv1a_and_the_colliding_pairs_collide holds them.
FULL_COLLISION = ((b"x-col", b"tk9b91fz"), (b"x-col", b"erb36pz0"))  # two fields, one full hash (and one name)
NAME_COLLISION = (b"x-hu70epuo", b"x-2tfo0yw8")                        # two names, one name hash


def _words(rows):
    return b"".join(int(w).to_bytes(4, "little") for r in rows for w in r)


def bw_bytes(bw):
    return b"".join(off.to_bytes(8, "little") + ln.to_bytes(4, "little") + nf.to_bytes(4, "little") for off, ln, nf in bw)


class Input:
    """a block table, a field table and a string arena in device memory"""

    def __init__(self, g, blocks, fields, arena):
        self.n = (len(blocks), len(fields), len(arena))
        self.blocks = g.DeviceBuffer(data=_words(blocks) + bytes(16))
        self.fields = g.DeviceBuffer(data=_words(fields) + bytes(16))
        self.strings = g.DeviceBuffer(data=bytes(arena) + bytes(16))

    def args(self):
        return (self.blocks.ptr, self.n[0], self.fields.ptr, self.n[1], self.strings.ptr, self.n[2])


class Wire:
    """a wire arena and a block-wire table filled with SENTINEL, with room behind the caps"""

    def __init__(self, g, wire_cap, bw_cap):
        self.caps = (wire_cap, bw_cap)
        self.wire = g.DeviceBuffer(data=bytes([SENTINEL]) * (wire_cap + 64))
        self.bw = g.DeviceBuffer(data=bytes([SENTINEL]) * (16 * (bw_cap + 4)))

    def args(self):
        return (self.wire.ptr, self.caps[0], self.bw.ptr, self.caps[1])


class HE:
    def __init__(self, g, table=4096, max_frame=16384):
        from grpc_rdma_amd import h2dev
        self.g = g
        self.enc = h2dev.HeaderEncoder(table, max_frame)
        self.model = HpencModel(table, max_frame)
        self.check()

    def set_peer(self, table, max_frame=16384):
        self.enc.set_peer(table, max_frame)
        self.model.set_peer(table, max_frame)

    def encode(self, lists=None, raw=None, wire_cap=None, bw_cap=None, device=None):
        """one call on the device and in the model, everything compared -> (wire bytes, block-wire table, result tuple).
        lists: [(stream, flags, [(name, value[, hint])])], or raw: (blocks, fields, arena) as they are; the caps default
        to what the call needs and 8 bytes, one entry more.  device: the six input arguments where the three tables
        stand in device memory already (raw: what they hold)"""
        import copy
        import pytest
        from tests.h2_device_lib import same
        blocks, fields, arena = pack(lists) if raw is None else raw
        if wire_cap is None or bw_cap is None:
            need = copy.deepcopy(self.model).encode(blocks, fields, arena, 1 << 40, 1 << 40)[2]
            wire_cap = need[2] + 8 if wire_cap is None else wire_cap
            bw_cap = need[0] + 1 if bw_cap is None else bw_cap
        wire, bw, res, err = self.model.encode(blocks, fields, arena, wire_cap, bw_cap)
        inp, out = None if device else Input(self.g, blocks, fields, arena), Wire(self.g, max(1, wire_cap), max(1, bw_cap))
        args = tuple(device or inp.args()) + out.args()
        if err:
            with pytest.raises(self.g.GrdmaError, match=ERR5 if err == "capacity" else ERR2):
                self.enc.encode(*args)
            got = self.enc.last_result
        else:
            n, got = self.enc.encode(*args)
            same(n, res[1], "encode: the frame count")
        print("encode: %r -> %r" % (res, got))
        same(got, res, "encode: result")
        w, b = out.wire.read(), out.bw.read()
        same(w, wire + bytes([SENTINEL]) * (len(w) - len(wire)), "encode: the whole wire arena")
        same(b, bw_bytes(bw) + bytes([SENTINEL]) * (len(b) - 16 * len(bw)), "encode: the whole block-wire table")
        self.check()
        return wire, bw, res

    def check(self):
        from tests.h2_device_lib import same
        t = self.model.table
        entries, info = self.enc.table()
        same(entries, t.entries, "the dynamic table, newest first")
        same(info, (len(t.entries), t.size, t.max_size), "the table's (entries, bytes, size limit)")
        st = self.enc.stats()
        same({k: st[k] for k in self.model.stats}, self.model.stats, "counters (all: %r)" % (st,))

    def close(self):
        self.enc.close()


# ---- strings for the cases --------------------------------------------------------------------------------------------------
def huffman_bits(data):
    return sum(HUFFMAN[b][1] for b in data)


def by_bits(nbits):
    """a byte value whose code has nbits bits"""
    return next(s for s in range(256) if HUFFMAN[s][1] == nbits)


def fill(n, stem=b"k"):
    """n distinct fields that match nothing static: for filling a table or a step of the walk"""
    return [(b"x-%s%04d" % (stem, i), b"v%04d" % i) for i in range(n)]


def chunk_lists(n, hint=2):
    """one block of n fields that insert nothing (hint 2, no match)"""
    return [(1, 0, [(nm, v, hint) for nm, v in fill(n)])]


assert CHUNK == 256
