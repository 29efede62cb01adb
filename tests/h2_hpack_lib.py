"""What the HPACK tests share (tests/test_h2_hpack_model.py, tests/test_zz_gpu_h2_hpack.py, tools/gen_hpack_vectors.py,
tools/h2_hpack_probe.py): a small HPACK *encoder* for the shapes no real encoder emits, a ctypes binding of nghttp2's
public hd API (an independent HPACK implementation; None where the library cannot be loaded), and the harness of the
device tests: a device parser with its header decoder (h2dev.HeaderDecoder), the oracle's parser and the model of
tests/h2_hpack_model.py beside them.  pytest rewrites no `assert` in a helper module: every check goes through `same`."""
import ctypes as C
import ctypes.util
import random

from tests.h2_hpack_model import HUFFMAN, STATIC, HpackModel

SENTINEL = 0xA5
ERR5 = "error 5"  # -GRDMA_ERR_CAPACITY


# ---- an encoder that does what it is told ---------------------------------------------------------------------------------
def enc_int(value, nbits, first=0, extra=0):
    """an integer with an nbits prefix under the pattern bits `first`; extra: that many more continuation bytes than
    needed (a non-minimal encoding; an integer below the prefix's limit is then written as limit + continuation)"""
    limit = (1 << nbits) - 1
    if value < limit and not extra:
        return bytes([first | value])
    out, rest = [first | limit], value - limit
    if rest < 0:
        raise ValueError("a non-minimal form exists only from the prefix's limit on")
    while rest >= 128:
        out.append(0x80 | (rest & 0x7f))
        rest >>= 7
    out.append(rest)
    for _ in range(extra):
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def huff(data, pad_bits=None, pad_ones=True):
    """the Huffman form of data; pad_bits: that many padding bits (a multiple of 8 above what fills the last byte is
    possible: 8 bits of padding is a whole byte of it), pad_ones False: zeros"""
    acc = n = 0
    for b in data:
        code, ln = HUFFMAN[b]
        acc, n = (acc << ln) | code, n + ln
    fill = (-n) % 8
    if pad_bits is not None:
        if (pad_bits - fill) % 8:
            raise ValueError("padding of %d bits does not end on a byte (%d would)" % (pad_bits, fill))
        fill = pad_bits
    acc = (acc << fill) | (((1 << fill) - 1) if pad_ones else 0)
    return acc.to_bytes((n + fill) // 8, "big")


def enc_str(data, h=False, **kw):
    body = huff(data, **kw) if h else bytes(data)
    return enc_int(len(body), 7, 0x80 if h else 0) + body


def indexed(i, extra=0):
    return enc_int(i, 7, 0x80, extra)


def literal(name, value, mode=1, hn=False, hv=False, extra=0):
    """mode 1 incremental, 2 without indexing, 3 never indexed; name: bytes, or the index of the entry that has it"""
    first, nbits = {1: (0x40, 6), 2: (0x00, 4), 3: (0x10, 4)}[mode]
    if isinstance(name, int):
        return enc_int(name, nbits, first, extra) + enc_str(value, hv)
    return bytes([first]) + enc_str(name, hn) + enc_str(value, hv)


def size_update(n, extra=0):
    return enc_int(n, 5, 0x20, extra)


def static_index(name, value=None):
    return next(i for i, (n, v) in enumerate(STATIC) if i and n == name and (value is None or v == value))


def random_headers(rng, n=None):
    """a header list whose names and values repeat often enough for a dynamic table to matter"""
    names = [b":path", b":authority", b"grpc-timeout", b"user-agent", b"x-trace", b"te", b"content-type", b"x-k%d" % rng.randrange(6)]
    out = []
    for _ in range(rng.randrange(1, 12) if n is None else n):
        name = rng.choice(names)
        r = rng.random()
        if r < 0.4:
            value = rng.choice([b"/svc/Method", b"trailers", b"application/grpc", b"10S", b"", b"a" * 40])
        elif r < 0.8:
            value = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789-/_.") for _ in range(rng.randrange(0, 60)))
        else:
            value = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 140)))
        out.append((name, value))
    return out


def own_block(rng, model_table, headers):
    """the list through this file's encoder, with random choices a real encoder does not make -> bytes.  model_table:
    the HpackTable the block will be decoded against (its dynamic entries are what may be referenced); it is updated as
    the encoder goes, so references to entries of this very block occur"""
    import copy
    t = copy.deepcopy(model_table)
    out = bytearray()
    for name, value in headers:
        full = [i for i in range(1, 62 + len(t.entries)) if t.get(i) == (name, value)]
        named = [i for i in range(1, 62 + len(t.entries)) if t.get(i)[0] == name]
        if full and rng.random() < 0.6:
            i = rng.choice(full)
            b = indexed(i, rng.choice([0, 1, 2]) if i >= 127 else 0)
        else:
            mode = rng.choice([1, 1, 2, 3])
            hn, hv = rng.random() < 0.5, rng.random() < 0.5
            if named and rng.random() < 0.7:
                i = rng.choice(named)
                b = literal(i, value, mode, hv=hv, extra=rng.choice([0, 1, 2]) if i >= (63 if mode == 1 else 15) else 0)
            else:
                b = literal(name, value, mode, hn, hv)
        out += b
        t.decode_block(bytes(b))
    return bytes(out)


# ---- nghttp2 ------------------------------------------------------------------------------------------------------------
class _NV(C.Structure):
    _fields_ = [("name", C.POINTER(C.c_uint8)), ("value", C.POINTER(C.c_uint8)), ("namelen", C.c_size_t),
                ("valuelen", C.c_size_t), ("flags", C.c_uint8)]


NO_INDEX = 1  # NGHTTP2_NV_FLAG_NO_INDEX


def _load():
    for name in ("libnghttp2.so.14", ctypes.util.find_library("nghttp2")):
        try:
            if name:
                lib = C.CDLL(name)
                lib.nghttp2_hd_inflate_hd2.restype = C.c_ssize_t
                lib.nghttp2_hd_inflate_hd2.argtypes = [C.c_void_p, C.POINTER(_NV), C.POINTER(C.c_int), C.c_char_p, C.c_size_t, C.c_int]
                lib.nghttp2_hd_deflate_hd.restype = C.c_ssize_t
                lib.nghttp2_hd_deflate_hd.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(_NV), C.c_size_t]
                lib.nghttp2_hd_deflate_bound.restype = C.c_size_t
                lib.nghttp2_hd_deflate_bound.argtypes = [C.c_void_p, C.POINTER(_NV), C.c_size_t]
                lib.nghttp2_hd_deflate_new.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
                lib.nghttp2_hd_inflate_new.argtypes = [C.POINTER(C.c_void_p)]
                for f in (lib.nghttp2_hd_deflate_change_table_size, lib.nghttp2_hd_inflate_change_table_size):
                    f.argtypes = [C.c_void_p, C.c_size_t]
                for f in (lib.nghttp2_hd_deflate_del, lib.nghttp2_hd_inflate_del, lib.nghttp2_hd_inflate_end_headers):
                    f.argtypes = [C.c_void_p]
                lib.nghttp2_hd_inflate_get_num_table_entries.restype = C.c_size_t
                lib.nghttp2_hd_inflate_get_num_table_entries.argtypes = [C.c_void_p]
                lib.nghttp2_hd_inflate_get_table_entry.restype = C.POINTER(_NV)
                lib.nghttp2_hd_inflate_get_table_entry.argtypes = [C.c_void_p, C.c_size_t]
                lib.nghttp2_hd_inflate_get_dynamic_table_size.restype = C.c_size_t
                lib.nghttp2_hd_inflate_get_dynamic_table_size.argtypes = [C.c_void_p]
                return lib
        except (OSError, AttributeError):
            pass
    return None


NGHTTP2 = _load()
NO_NGHTTP2 = "libnghttp2 cannot be loaded on this machine"


class Deflater:
    def __init__(self, table_size=4096):
        self.h = C.c_void_p()
        rc = NGHTTP2.nghttp2_hd_deflate_new(C.byref(self.h), table_size)
        if rc:
            raise RuntimeError("nghttp2_hd_deflate_new: %d" % rc)

    def change_table_size(self, n):
        rc = NGHTTP2.nghttp2_hd_deflate_change_table_size(self.h, n)
        if rc:
            raise RuntimeError("nghttp2_hd_deflate_change_table_size: %d" % rc)

    def deflate(self, headers, no_index=()):
        """headers: [(name, value)]; no_index: positions sent as never-indexed literals -> the block"""
        keep = [(C.create_string_buffer(n, max(1, len(n))), C.create_string_buffer(v, max(1, len(v)))) for n, v in headers]
        nva = (_NV * max(1, len(headers)))()
        for i, ((n, v), (bn, bv)) in enumerate(zip(headers, keep)):
            nva[i].name, nva[i].value = C.cast(bn, C.POINTER(C.c_uint8)), C.cast(bv, C.POINTER(C.c_uint8))
            nva[i].namelen, nva[i].valuelen, nva[i].flags = len(n), len(v), NO_INDEX if i in no_index else 0
        cap = NGHTTP2.nghttp2_hd_deflate_bound(self.h, nva, len(headers))
        buf = C.create_string_buffer(cap)
        n = NGHTTP2.nghttp2_hd_deflate_hd(self.h, buf, cap, nva, len(headers))
        if n < 0:
            raise RuntimeError("nghttp2_hd_deflate_hd: %d" % n)
        return buf.raw[:n]

    def __del__(self):
        if NGHTTP2 is not None and self.h:
            NGHTTP2.nghttp2_hd_deflate_del(self.h)


class Inflater:
    def __init__(self, setting=None):
        self.h = C.c_void_p()
        rc = NGHTTP2.nghttp2_hd_inflate_new(C.byref(self.h))
        if rc:
            raise RuntimeError("nghttp2_hd_inflate_new: %d" % rc)
        if setting is not None:
            self.change_table_size(setting)

    def change_table_size(self, n):
        rc = NGHTTP2.nghttp2_hd_inflate_change_table_size(self.h, n)
        if rc:
            raise RuntimeError("nghttp2_hd_inflate_change_table_size: %d" % rc)

    def inflate(self, block):
        """-> [(name, value, never indexed)], or None where nghttp2 rejects the block"""
        out, pos = [], 0
        while True:
            nv, flags = _NV(), C.c_int(0)
            n = NGHTTP2.nghttp2_hd_inflate_hd2(self.h, C.byref(nv), C.byref(flags), block[pos:], len(block) - pos, 1)
            if n < 0:
                return None
            pos += n
            if flags.value & 2:  # NGHTTP2_HD_INFLATE_EMIT
                out.append((bytes(nv.name[:nv.namelen]), bytes(nv.value[:nv.valuelen]), bool(nv.flags & NO_INDEX)))
            if flags.value & 1:  # NGHTTP2_HD_INFLATE_FINAL
                NGHTTP2.nghttp2_hd_inflate_end_headers(self.h)
                return out
            if n == 0 and pos >= len(block) and not flags.value & 2:
                return None

    def table(self):
        """the dynamic table, newest first, and its size"""
        n = NGHTTP2.nghttp2_hd_inflate_get_num_table_entries(self.h)
        out = []
        for i in range(62, n + 1):
            nv = NGHTTP2.nghttp2_hd_inflate_get_table_entry(self.h, i).contents
            out.append((bytes(nv.name[:nv.namelen]), bytes(nv.value[:nv.valuelen])))
        return out, NGHTTP2.nghttp2_hd_inflate_get_dynamic_table_size(self.h)

    def __del__(self):
        if NGHTTP2 is not None and self.h:
            NGHTTP2.nghttp2_hd_inflate_del(self.h)


def huffman_from_nghttp2():
    """RFC 7541 Appendix B as nghttp2 has it: the value bytes([s]) + b"0" * 40 through a deflater without table; behind
    the trailing 1-bits (the padding) and the 200 zero bits of the forty "0" (code 00000) stands the code of s"""
    codes = []
    for s in range(256):
        block = Deflater(0).deflate([(b"x", bytes([s]) + b"0" * 40)])
        while block[0] & 0xe0 == 0x20 and block[0] & 0x1f < 0x1f:  # (a deflater without table says so first: a size update)
            block = block[1:]
        first = block[0]
        if first & 0xf0 not in (0x00, 0x10, 0x40) or block[1] & 0x80 or block[1] != 1 or block[2:3] != b"x":
            raise RuntimeError("an unexpected literal form: %s" % block[:4].hex())
        pos = 3
        h, ln = block[pos] & 0x80, block[pos] & 0x7f
        pos += 1
        if ln == 0x7f:
            ln, shift = 0x7f, 0
            while True:
                ln += (block[pos] & 0x7f) << shift
                shift += 7
                pos += 1
                if not block[pos - 1] & 0x80:
                    break
        if not h:
            raise RuntimeError("symbol %d: the deflater did not use the Huffman form" % s)
        bits = int.from_bytes(block[pos:pos + ln], "big")
        nbits = 8 * ln
        while bits & 1:
            bits, nbits = bits >> 1, nbits - 1
        if bits & ((1 << 200) - 1):
            raise RuntimeError("symbol %d: no 200 zero bits behind the code" % s)
        codes.append((bits >> 200, nbits - 200))
    return codes + [(0x3fffffff, 30)]


# ---- the harness of the device tests ------------------------------------------------------------------------------------
def headers_frames(sid, block, flags=0, cont=(), pad=None, priority=False):
    """HEADERS (+ CONTINUATIONs cutting the block at the offsets `cont`) of one block; END_HEADERS on the last frame;
    flags: END_STREAM; pad: that many padding bytes behind the fragment (the PADDED flag), priority: 5 bytes in front"""
    from tests.h2_helpers import frame
    cuts = [0] + list(cont) + [len(block)]
    parts = [block[a:b] for a, b in zip(cuts, cuts[1:])]
    out = bytearray()
    for k, part in enumerate(parts):
        fl = 4 if k == len(parts) - 1 else 0
        if k == 0:
            fl |= flags | (8 if pad is not None else 0) | (0x20 if priority else 0)
            part = (bytes([pad]) if pad is not None else b"") + (b"\x80\x00\x00\x03\x10" if priority else b"") + part + bytes(pad or 0)
        out += frame(1 if k == 0 else 9, fl, sid, part)
    return bytes(out)


class Targets:
    """block table, field table and string arena filled with SENTINEL, with room behind the caps"""

    def __init__(self, g, blocks_cap, fields_cap, strings_cap):
        self.caps = (blocks_cap, fields_cap, strings_cap)
        self.blocks = g.DeviceBuffer(data=bytes([SENTINEL]) * (16 * (blocks_cap + 4)))
        self.fields = g.DeviceBuffer(data=bytes([SENTINEL]) * (16 * (fields_cap + 4)))
        self.strings = g.DeviceBuffer(data=bytes([SENTINEL]) * (strings_cap + 64))

    def read(self):
        return self.blocks.read(), self.fields.read(), self.strings.read()

    def args(self):
        return (self.blocks.ptr, self.caps[0], self.fields.ptr, self.caps[1], self.strings.ptr, self.caps[2])


def _words(rows):
    return b"".join(int(w).to_bytes(4, "little") for r in rows for w in r)


class HH:
    def __init__(self, g, prefix=False, streams=(), setting=4096, max_block=65536, caps=(512, 4096, 1 << 16)):
        from grpc_rdma_amd import h2dev
        from tests.h2_device_lib import ParserPair
        self.g, self.h2dev = g, h2dev
        self.pp = ParserPair(g, prefix, streams)
        self.parser = self.pp.dev
        self.dec = h2dev.HeaderDecoder(self.parser, setting, max_block)
        self.model = HpackModel(setting, max_block)
        self.caps = caps
        self.last, self.last_slices, self.buf = (0, []), [], None
        self.skipped = self.lost = False

    def deframe(self, slices, ev_cap=None, checked=True):
        """one standalone deframing on the device and in the oracle; the arena stays until the next one"""
        from tests.h2_device_lib import same
        self.buf, table = self.pp.upload(slices)
        self.last, self.last_slices = self.pp.expect(slices), slices
        got = self.parser.deframe(self.buf.ptr, table, cap=ev_cap or 8 * len(slices) + 4096)
        if checked:
            same(got[0], self.last[0], "h2 error")
            same(got[1], self.last[1], "events")
        return got

    def set_max_table_size(self, n):
        self.dec.set_max_table_size(n)
        self.model.set_max_table_size(n)
        self.check()

    def decode(self, caps=None):
        """decode the last deframing on the device and in the model, compare everything -> (blocks, result): blocks as
        [(stream, flags, [(name, value, representation)])]"""
        import pytest
        from tests.h2_device_lib import same
        caps = caps or self.caps
        t = self.target = Targets(self.g, *caps)
        err_o, ev_o = self.last
        blocks, fields, strings, res, rc = self.model.decode(ev_o, self.last_slices, err_o, caps, skipped=self.skipped, lost=self.lost)
        if res[7] != 1:
            self.skipped = self.lost = False
        if rc:
            with pytest.raises(self.g.GrdmaError, match=ERR5):
                self.dec.decode(*t.args())
            got = self.dec.last_result
        else:
            n, got = self.dec.decode(*t.args())
            same(n, len(blocks), "decode: the block count")
        print("decode: %r -> %r" % (res, got))
        same(got, res, "decode: result")
        b, f, s = t.read()
        same(b, _words(blocks) + bytes([SENTINEL]) * (len(b) - 16 * len(blocks)), "decode: the whole block table")
        same(f, _words(fields) + bytes([SENTINEL]) * (len(f) - 16 * len(fields)), "decode: the whole field table")
        same(s, strings + bytes([SENTINEL]) * (len(s) - len(strings)), "decode: the whole string arena")
        self.check()
        out = []
        for stream, first, n, flags in blocks:
            out.append((stream, flags, [(strings[no:no + (nl & 0xffffff)], strings[vo:vo + vl], nl >> 24)
                                         for no, vo, nl, vl in fields[first:first + n]]))
        return out, res

    def feed(self, slices, ev_cap=None, caps=None):
        self.deframe(slices, ev_cap)
        return self.decode(caps)

    def check(self):
        from tests.h2_device_lib import same
        entries, info = self.dec.table()
        same(entries, self.model.table.entries, "the dynamic table, newest first")
        same(info, (len(self.model.table.entries), self.model.table.size, self.model.table.max_size),
             "the table's (entries, bytes, size limit)")
        st = self.dec.stats()
        same({k: st[k] for k in self.model.stats}, self.model.stats, "counters (all: %r)" % (st,))

    def close(self):
        self.dec.close()
        self.parser.close()


def capture_blocks():
    """the header blocks of tests/golden/h2_grpcio_capture.json, in order: [(stream, block)] (no frame of it is padded)"""
    import json
    import os
    d = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "h2_grpcio_capture.json")))
    wire = bytes.fromhex(d["client_bytes_hex"])[24:]
    out, pos, cur = [], 0, None
    while pos < len(wire):
        n, t, fl, sid = int.from_bytes(wire[pos:pos + 3], "big"), wire[pos + 3], wire[pos + 4], int.from_bytes(wire[pos + 5:pos + 9], "big")
        body = wire[pos + 9:pos + 9 + n]
        if t == 1:
            if fl & 0x28:
                raise RuntimeError("a padded or prioritised HEADERS frame in the capture")
            cur = [sid, bytearray(body)]
        elif t == 9:
            cur[1] += body
        if t in (1, 9) and fl & 4:
            out.append((cur[0], bytes(cur[1])))
        pos += 9 + n
    return out


# ---- cases shared by tests/test_h2_hpack_model.py and tools/gen_hpack_vectors.py ------------------------------------------
def deflated_sequence(seed, nblocks=4):
    """header lists through nghttp2's deflater at table sizes 0, 100 and 4096, with changes of the size between blocks
    and some fields flagged NGHTTP2_NV_FLAG_NO_INDEX -> [(block, headers, positions never indexed)]"""
    rng = random.Random(seed)
    d = Deflater(rng.choice([0, 100, 4096]))
    out = []
    for _ in range(nblocks):
        if rng.random() < 0.3:
            d.change_table_size(rng.choice([0, 100, 4096]))
        headers = random_headers(rng)
        never = {i for i in range(len(headers)) if rng.random() < 0.15}
        out.append((d.deflate(headers, never), headers, never))
    return out


def own_sequence(seed, nblocks=4):
    """header lists through this file's encoder against a model table of its own -> [(block, headers)]"""
    from tests.h2_hpack_model import HpackTable
    rng = random.Random(seed)
    t, out = HpackTable(), []
    for k in range(nblocks):
        headers = random_headers(rng)
        lead = b""
        if rng.random() < 0.3:
            sizes = [rng.choice([0, 64, 300, 4096]) for _ in range(rng.randrange(1, 3))]
            lead = b"".join(size_update(n, rng.choice([0, 0, 1]) if n >= 31 else 0) for n in sizes)
            t.decode_block(lead)
        block = lead + own_block(rng, t, headers)
        t.decode_block(block[len(lead):])
        out.append((block, headers))
    return out


def malformed():
    """[(what, blocks in front of it, the block)]: each rejected by the model and by nghttp2"""
    fill = literal(b"a", b"1")
    return [
        ("index 0", [], b"\x82\x80"),
        ("an index beyond the table", [fill], indexed(63)),
        ("ten 0xff continuation bytes", [], b"\xff" + b"\xff" * 10 + b"\x00"),
        ("EOS", [], b"\x00\x01k" + enc_int(4, 7, 0x80) + (0x3fffffff << 2 | 3).to_bytes(4, "big")),
        ("8 bits of padding", [], b"\x00\x01k" + enc_int(6, 7, 0x80) + huff(b"00000000", pad_bits=8)),
        ("a zero bit in the padding", [], b"\x00\x01k" + enc_int(1, 7, 0x80) + huff(b"0", pad_bits=3, pad_ones=False)),
        ("a string past the block's end", [], b"\x82\x00\x01a\x05abcd"),
        ("a size update behind a field", [], b"\x82" + size_update(100)),
        ("a size update above the setting", [], size_update(4097) + b"\x82"),
    ]
