"""Shared by tests/test_zz_gpu_movers.py and tests/test_movers_emu.py: the case lists of the mover sweep, the memcpy
reference (plain numpy, nothing of the code under test) and the driver of tests/cc/mover_sweep.hip.

Every list is generated from the code's own boundaries (16-byte units, 64 lanes, U registers per lane, tile size,
GRDMA_MAX_SEGS, the LDS slots of the sampled prefix), never sampled at random.  A length above what a mover's
registers hold (wave_move_tile: 1024 * U, tiny: 64) is outside that mover's contract and is not generated."""
import bisect
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "grpc-rdma_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cc", "mover_sweep.hip")
DEPS = [SRC, os.path.join(CSRC, "grdma_devfn.h"), os.path.join(CSRC, "grdma_dev.h")]
EMU_DEPS = DEPS + [os.path.join(ROOT, "tests", "cc", "wave_emu.h"), os.path.join(ROOT, "tests", "cc", "hip_api_emu.h")]
SO_GPU = os.path.join(ROOT, "oracle", "_build", "libmover_sweep.so")
SO_EMU = os.path.join(ROOT, "oracle", "_build", "libmover_sweep_emu.so")

MAX_SEGS = 16384                       # GRDMA_MAX_SEGS
ZERO_SRC, TAG_HDR, TAG_FTR, TAG_WRITE, TAG_LEN_SHIFT = 1, 2, 4, 8, 8
FOOTER = 0xFFFFFFFFFFFFFFFF
NULL_SRC = 0xFFFFFFFFFFFFFFFF          # "zero-fill segment" in the entry's segment table

VARIANTS = ["copy", "copy_null", "copy_g", "copy_g_null", "zero", "move8", "move16", "move8_z", "move16_z", "tiny", "tiny_z"]
VID = {v: i for i, v in enumerate(VARIANTS)}
# what the variant promises (copy_g: as documented)
CAP = {"copy": 8192, "copy_null": 8192, "copy_g": 8192, "copy_g_null": 8192, "zero": 16384, "move8": 8192, "move16": 16384,
       "move8_z": 8192, "move16_z": 16384, "tiny": 64, "tiny_z": 64}
HARD_CAP = {"move8", "move16", "move8_z", "move16_z", "tiny", "tiny_z"}   # the registers hold no more
HAS_SRC = {"copy", "copy_g", "move8", "move16", "move8_z", "move16_z", "tiny", "tiny_z"}
CLEARS_SRC = {"move8_z", "move16_z", "tiny_z"}

UNIT_EDGES = [0, 1, 2, 7, 8, 9, 15, 16, 17, 30, 31, 32, 33, 47, 48, 63, 64, 65]


class case_struct(C.Structure):
    _fields_ = [("variant", C.c_uint32), ("n", C.c_uint32), ("d", C.c_uint64), ("s", C.c_uint64)]


def build(emulated):
    """Builds the harness when it is missing or older than its sources; returns the loaded library."""
    so, deps = (SO_EMU, EMU_DEPS) if emulated else (SO_GPU, DEPS)
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        if emulated:
            cmd = [CLANG, "-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17", "-fPIC", "-pthread", "-Wno-unused-value",
                   "-Wno-unknown-attributes", "-Wno-ignored-attributes", "-I" + os.path.join(ROOT, "tests", "cc"),
                   "-I" + os.path.join(ROOT, "tests", "cc", "emu_include"), "-x", "c++", "-shared", SRC, "-o", so]
        else:
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-shared", SRC, "-o", so]
        subprocess.check_call(cmd)
    L = C.CDLL(so)
    L.ms_run_tiles.restype = C.c_int64
    L.ms_run_tiles.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(case_struct), C.c_uint32, C.c_uint32]
    L.ms_run_plan.restype = C.c_int64
    L.ms_run_plan.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                              C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.c_uint64, C.c_uint64]
    L.ms_margin.restype = C.c_uint64
    L.ms_margin.argtypes = [C.c_int]
    return L


def pattern(n, salt):
    """Position-dependent bytes without a zero and without a period of 1, 16 or 64 (steps of 7, 125 and 19 mod 255)."""
    have = _PATTERNS.get(salt)
    if have is None or have.size < n:       # (a prefix of a longer pattern is the shorter one)
        i = np.arange(max(n, 4 << 20), dtype=np.uint64)
        x = i * 7 + (i >> 4) * 13 + (i >> 6) * 29 + (i >> 10) * 31 + (i >> 16) * 37 + salt
        have = _PATTERNS[salt] = (1 + x % 255).astype(np.uint8)
    return have[:n].copy()


_PATTERNS = {}


# ---- the one-wave cases -----------------------------------------------------------------------------------------
def boundary_lengths(variant, head):
    """Lane-63 / per-lane-register boundaries, each +-1 and +-16, and each also plus `head`, so that `units` itself
    lands on the boundary whatever the destination alignment; then the end of the variant's promise."""
    cap = CAP[variant]
    out = set()
    for b in (1024, 2048, 3072, 4096, 4112, 4113, cap):   # (cap == 1024 * U for the movers with registers)
        for delta in (-16, -1, 0, 1, 16):
            out.update((b + delta, b + delta + head))
    out.update((cap - 17, cap - 16, cap - 15, cap - 1, cap))
    if variant.startswith("copy"):
        out.update((cap + 1, cap + 4097))                     # the loop fall-back
    return out


def lengths(variant, head, boundaries_only=False):
    out = boundary_lengths(variant, head)
    if not boundaries_only:
        out.update(UNIT_EDGES)
        out.update(range(1, 32))                              # the zero-behind branch switch of wave_move_tile
    if variant in HARD_CAP:
        out = {n for n in out if n <= CAP[variant]}
    return sorted(n for n in out if n >= 0)


def alignments(variant):
    return [(d, s) for d in range(16) for s in range(16)] if variant in HAS_SRC else [(d, 0) for d in range(16)]


RULE_PAIRS = sorted({(0, 0)} | {(0, s) for s in range(16)} | {(d, 0) for d in range(16)} | {(d, d) for d in range(16)} |
                    {(d, (16 - d) & 15) for d in range(16)})


def tile_cases(variant, subset=False):
    """[(variant, d & 15, s & 15, n)].  Full list: every alignment pair x every length.  subset (the rule for the
    emulated run): every alignment pair at every boundary length for copy_g and the movers with registers, every length
    at the pairs (0,0), (0,s), (d,0), (d,d), (d,16-d)."""
    out = []
    for d, s in alignments(variant):
        head = (16 - d) & 15
        if not subset or (d, s) in RULE_PAIRS or variant not in HAS_SRC:
            ns = lengths(variant, head)
        elif variant == "copy_g" or variant.startswith("move"):
            ns = lengths(variant, head, boundaries_only=True)
        else:
            continue
        out += [(variant, d, s, n) for n in ns]
    return out


GAP = 80          # canary bytes between the windows of two cases (the slot stays a multiple of 16)
CHUNK = 24 << 20  # bytes of one pool per launch


def run_tile_cases(L, cases, threads=256):
    """Lays the cases out in chunks, runs each chunk in one launch and compares both pools, whole, with the reference.
    Returns the number of cases run."""
    margin = int(L.ms_margin(0))
    ran, i = 0, 0
    while i < len(cases):
        cur_d = cur_s = margin
        placed = []
        while i < len(cases) and max(cur_d, cur_s) < CHUNK:
            v, d, s, n = cases[i]
            placed.append((v, cur_d + d, cur_s + s, n))
            slot = ((n + 15 + 15) & ~15) + GAP
            cur_d += slot
            cur_s += slot
            i += 1
        dlen, slen = cur_d + margin, cur_s + margin
        d0, s0 = pattern(dlen, 101), pattern(slen, 0)
        exp_d, exp_s = d0.copy(), s0.copy()
        for v, d, s, n in placed:
            exp_d[d:d + n] = s0[s:s + n] if v in HAS_SRC else 0
            if v in CLEARS_SRC:
                exp_s[s:s + n] = 0
        got_d, got_s = d0.copy(), s0.copy()
        table = (case_struct * len(placed))(*[case_struct(VID[v], n, d, s) for v, d, s, n in placed])
        rc = L.ms_run_tiles(got_d.ctypes.data, dlen, got_s.ctypes.data, slen, table, len(placed), threads)
        assert rc == len(placed), "ms_run_tiles returned %d for %d cases" % (rc, len(placed))
        _compare(exp_d, got_d, "destination", [(c[1], c) for c in placed])
        _compare(exp_s, got_s, "source", [(c[2], c) for c in placed])
        ran += len(placed)
    return ran


def _compare(exp, got, pool, windows):
    if np.array_equal(exp, got):
        return
    bad = np.flatnonzero(exp != got)
    first = int(bad[0])
    starts = [w[0] for w in windows]
    k = max(0, bisect.bisect_right(starts, first) - 1)
    # (a byte in front of window k + 1 may belong to it: name the nearer one)
    if k + 1 < len(windows) and first >= starts[k] + windows[k][1][3] + GAP // 2:
        k += 1
    v, d, s, n = windows[k][1]
    raise AssertionError("%s d=%d s=%d n=%d: the %s pool first differs at offset %d of the case's window (pool offset %d): "
                         "expected 0x%02x, got 0x%02x; %d bytes differ in this launch"
                         % (v, d & 15, s & 15, n, pool, first - starts[k], first, exp[first], got[first], bad.size))


# ---- plans ------------------------------------------------------------------------------------------------------
def shift_of(nsegs, lds_n):
    sh = 0
    while ((nsegs >> sh) + 1) > lds_n:
        sh += 1
    return sh


class Plan:
    """A plan over two pools.  add() places a segment at the next free place; a ring (wrap=True) puts the tag side of
    every segment into a power-of-two window instead, at the ring offset the caller names."""

    def __init__(self, name, tile, margin, ring=None, ring_pool=0):
        self.name, self.tile, self.margin = name, tile, margin
        self.cur = [margin, margin]          # next free byte of the destination / source pool
        self.segs = []                       # (dst, src or None, len, flags)
        self.ring, self.ring_pool = ring, ring_pool
        if ring:
            self.ring_off = self.cur[ring_pool]
            self.cur[ring_pool] += ring + 256

    def _place(self, pool, n, align):
        at = self.cur[pool] + 32 + align     # (room for a header word in front, padding + footer behind)
        self.cur[pool] = (at + n + 15 + 48 + 15) & ~15
        return at

    def add(self, n, flags=0, zero_fill=False, da=0, sa=0, ring_at=None):
        wr = bool(flags & TAG_WRITE)
        tagged = bool(flags & (TAG_HDR | TAG_FTR))
        if tagged:   # records are 8-aligned on the side that carries the tags
            if wr:
                da &= 8
            else:
                sa &= 8
        if flags & TAG_WRITE:
            flags |= n << TAG_LEN_SHIFT
        if ring_at is not None:
            side = self.ring_off + ring_at
            dst = side if self.ring_pool == 0 else self._place(0, n, da)
            src = side if self.ring_pool == 1 else self._place(1, n, sa)
        else:
            dst = self._place(0, n, da)
            src = None if zero_fill else self._place(1, n, sa)
        self.segs.append((dst, src, n, flags))

    def prefix(self):
        p = [0]
        for _, _, n, _ in self.segs:
            p.append(p[-1] + (n + self.tile - 1) // self.tile)
        return p


def reference_plan(plan, d0, s0):
    exp = [d0.copy(), s0.copy()]
    tag_off, tm = (plan.ring_off, plan.ring - 1) if plan.ring else (0, (1 << 64) - 1)

    def put64(pool, at, v):
        exp[pool][at:at + 8] = np.frombuffer(int(v).to_bytes(8, "little"), dtype=np.uint8)

    for dst, src, n, flags in plan.segs:
        exp[0][dst:dst + n] = s0[src:src + n] if src is not None else 0
        if src is not None and flags & ZERO_SRC:
            exp[1][src:src + n] = 0
        if flags & (TAG_HDR | TAG_FTR):
            wr = bool(flags & TAG_WRITE)
            pool, side = (0, dst) if wr else (1, src)
            if flags & TAG_HDR:
                put64(pool, tag_off + ((side - 8 - tag_off) & tm), (flags >> TAG_LEN_SHIFT) if wr else 0)
            if flags & TAG_FTR:
                e = (side + n - tag_off) & tm
                pad = (0 - e) & 7
                exp[pool][tag_off + e:tag_off + e + pad] = 0
                put64(pool, tag_off + ((e + pad) & tm), FOOTER if wr else 0)
    return exp


def run_plan_case(L, plan, kind, grid):
    """kind 0: run_plan<256, true>, 1: run_plan<256, false>, 2: run_plan<1024, true> in one plan workgroup."""
    dlen, slen = plan.cur[0] + plan.margin, plan.cur[1] + plan.margin
    d0, s0 = pattern(dlen, 101), pattern(slen, 0)
    exp_d, exp_s = reference_plan(plan, d0, s0)
    got_d, got_s = d0.copy(), s0.copy()
    n = len(plan.segs)
    flat = []
    for dst, src, ln, flags in plan.segs:
        flat += [dst, NULL_SRC if src is None else src, ln, flags]
    pre = plan.prefix()
    rc = L.ms_run_plan(kind, grid, got_d.ctypes.data, dlen, got_s.ctypes.data, slen, (C.c_uint64 * len(flat))(*flat), n,
                       (C.c_uint32 * len(pre))(*pre), plan.tile, plan.ring_pool if plan.ring else 0,
                       plan.ring_off if plan.ring else 0, (plan.ring - 1) if plan.ring else (1 << 64) - 1)
    assert rc == n, "ms_run_plan returned %d for %d segments (%s)" % (rc, n, plan.name)
    for pool, exp, got, col in (("destination", exp_d, got_d, 0), ("source", exp_s, got_s, 1)):
        if np.array_equal(exp, got):
            continue
        bad = np.flatnonzero(exp != got)
        first = int(bad[0])
        wins = sorted((sg[col], i) for i, sg in enumerate(plan.segs) if sg[col] is not None)
        k = max(0, bisect.bisect_right([w[0] for w in wins], first + 16) - 1)
        i = wins[k][1]
        dst, src, ln, flags = plan.segs[i]
        raise AssertionError("plan %s kind=%d grid=%d tile=%d nsegs=%d ntiles=%d: the %s pool first differs at pool offset %d, "
                             "offset %d of segment %d (d=%d s=%s n=%d flags=0x%x): expected 0x%02x, got 0x%02x; %d bytes differ"
                             % (plan.name, kind, grid, plan.tile, n, pre[-1], pool, first, first - wins[k][0], i, dst & 15,
                                "null" if src is None else src & 15, ln, flags, exp[first], got[first], bad.size))
    return 1


TINY = [1, 9, 63, 64]


def plan_cases(L):
    """[(Plan, kind, grid)]: every plan case of the sweep."""
    margin = int(L.ms_margin(1))
    out = []
    for tile in (8192, 16384):
        shapes = [(0, 1), (0, 2), (0, 8), (1, 1), (1, 2), (1, 8), (2, 1)]   # (kind, grid); 8 workgroups: idle waves
        for kind, grid in shapes:
            nwaves = 4 if kind == 2 else 4 * grid
            # -- one tile per segment (the pair path)
            for count in (1, 2, 3, 4 * nwaves + 1):
                p = Plan("one-tile x%d" % count, tile, margin)
                for i in range(count):
                    p.add([65, tile, 100, tile - 1, 4113, 1000][i % 6], flags=ZERO_SRC if i % 3 == 1 else 0, da=(5 * i + 3) & 15, sa=(11 * i + 7) & 15)
                out.append((p, kind, grid))
            p = Plan("tiny places", tile, margin)
            i = 0
            for t in TINY:
                for flavour in ("plain", "zero_src", "zero_fill"):
                    for a, b in ((t, 65), (65, t), (t, t), (65, 65)):   # tiny in the even place, the odd place, both, neither
                        for n in (a, b):
                            p.add(n, flags=ZERO_SRC if flavour == "zero_src" else 0, zero_fill=flavour == "zero_fill",
                                  da=(5 * i + 1) & 15, sa=(3 * i + 2) & 15)
                            i += 1
            out.append((p, kind, grid))
            # -- tags, linear window: every padding, header only / footer only / both, sender and receiver form
            p = Plan("tags linear", tile, margin)
            q = Plan("tags linear + multi-tile", tile, margin)
            q.add(3 * tile + 5, flags=TAG_HDR | TAG_FTR | TAG_WRITE)     # header and footer written by different tiles
            for pay in list(range(1, 18)) + list(range(65, 82)):
                for bits in (TAG_HDR, TAG_FTR, TAG_HDR | TAG_FTR):
                    for wr in (TAG_WRITE, 0):
                        for plan_ in (p, q):
                            plan_.add(pay, flags=bits | wr | (ZERO_SRC if not wr and pay % 2 else 0), da=(pay * 3) & 15, sa=(pay * 5) & 15)
            q.add(tile + 1, flags=TAG_HDR | TAG_FTR | ZERO_SRC)
            out += [(p, kind, grid), (q, kind, grid)]
            # -- tags in a ring: a record whose footer lands at ring offset 0, one whose header wraps to the ring's end
            for ring_pool, wr in ((0, TAG_WRITE), (1, 0)):
                for pay in (1, 8, 17, 65, 200):
                    ring = 4096
                    p = Plan("tags ring footer@0 pay=%d pool=%d" % (pay, ring_pool), tile, margin, ring=ring, ring_pool=ring_pool)
                    p.add(pay, flags=TAG_HDR | TAG_FTR | wr, ring_at=ring - ((pay + 7) & ~7), sa=3, da=5)
                    p.add(100, flags=TAG_HDR | TAG_FTR | wr, ring_at=16, sa=9, da=2)
                    out.append((p, kind, grid))
                    p = Plan("tags ring header@end pay=%d pool=%d" % (pay, ring_pool), tile, margin, ring=ring, ring_pool=ring_pool)
                    p.add(pay, flags=TAG_HDR | TAG_FTR | wr, ring_at=0, sa=1, da=7)
                    p.add(3000, flags=TAG_HDR | TAG_FTR | wr, ring_at=512, sa=6, da=4)
                    p.add(1, flags=0)
                    p.add(tile + 9, flags=0)     # (general path in the ring case as well)
                    out.append((p, kind, grid))
        # -- segment counts at the clamps of the descriptor prefetch (one tile per segment) and every value of `shift`
        #    of the sampled prefix (general path); the big counts under one grid per kind
        for kind, grid in ((0, 2), (1, 2), (2, 1)):
            for count in (MAX_SEGS - 1, MAX_SEGS):
                p = Plan("one-tile x%d" % count, tile, margin)
                for i in range(count):
                    p.add([1, 9, 65, 63, 64, 100, 17, 300][i % 8] if i % 1021 else tile, flags=ZERO_SRC if i % 5 == 2 else 0,
                          zero_fill=i % 7 == 3, da=(5 * i + 3) & 15, sa=(11 * i + 7) & 15)
                out.append((p, kind, grid))
        for count in (2, 255, 256, 257, 511, 512, 513, 1024, 4097, MAX_SEGS - 1, MAX_SEGS):
            multi = {0, count - 1, count // 2}
            for lds_n in (256, 1024):
                stride = 1 << shift_of(count, lds_n)
                for k in (0, (count // stride) // 2, (count - 1) // stride):      # first, middle and last stride
                    for j in (stride // 2 + 1, 3 * stride // 4, stride - 1):      # upper half of the stride
                        if stride > 1 and k * stride + j < count:
                            multi.add(k * stride + j)
            big = sorted(multi)
            p = Plan("general x%d" % count, tile, margin)
            for i in range(count):
                if i in multi:
                    n = [3 * tile + 5, tile + 1][big.index(i) % 2]
                    flags = [0, ZERO_SRC, TAG_HDR | TAG_FTR | TAG_WRITE][big.index(i) % 3]
                elif i - 1 in multi or (i - 2 in multi and big.index(i - 2) % 2 == 0):
                    n, flags = 0, 0        # segments without a tile behind a multi-tile one: the walk steps over them
                elif i % 509 == 7:
                    n, flags = [tile - 1, tile][(i // 509) % 2], 0
                else:
                    n, flags = [1, 9, 65, 63, 64, 100, 17, 300][i % 8], (ZERO_SRC if i % 5 == 2 else 0)
                p.add(n, flags=flags, zero_fill=(i % 7 == 3 and i not in multi and n > 0), da=(5 * i + 3) & 15, sa=(11 * i + 7) & 15)
            assert p.prefix()[-1] > count                                        # (not the one-tile-per-segment path)
            shapes = [(0, 1), (0, 2), (0, 8), (1, 1), (1, 2), (1, 8), (2, 1)] if count <= 1024 else [(0, 2), (1, 2), (2, 1)]
            out += [(p, kind, grid) for kind, grid in shapes]
    return out
