"""TEST INFRASTRUCTURE: the latency engine's one-wave send and drain at their edges.

The unary round trip runs through three one-wave code paths: the watcher's single-wave drain (rxw_fast,
csrc/grdma_engine_kernels.inc), the unary branch of tx_small_wave (csrc/grdma_tx_body.h) and the Send straight from
the doorbell wave (engine_body -> tx_small_direct).  This module builds message sequences from the constants those
paths branch on, drives `pyorc.OracleLink` through them and records, for every drain, the state in front of it, the
records it will see, the endpoint reads it must deliver -- and whether the single-wave path TAKES it, from a plain
Python predicate restated from the guards and comments of rxw_fast and express_fits and fed oracle state only.  A drain
that wrongly declines is delivered by the plan body with the same bytes: only the exact count shows it.

`Seq` is builder and reference in one: every `msg` / `group` runs the oracle at once, so the steering helpers
(`to_head`, `to_irs`, `to_leftover`) read head, internal_read_size and leftover_cap from the oracle itself.
`run_on_device` replays a finished `Seq` on a connection a -> b of the product library.  `check_cases` evaluates every
case's witnesses on the oracle's trace alone; tests/test_zzz_gpu_latency_sweep.py calls it at import, so a case that
misses its edge fails collection on any machine.

Only tests/ may import this module."""
import ctypes as C
import os
import subprocess
import tempfile
import time

from oracle import pyorc
from tests.pair_lib import STATE_KEYS, mk_link

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grpc-rdma_amd", "csrc")

MAX_SGE = 30            # records per Send (the reference's default): a message of the sweep is at most this many
MAX_MESSAGES = 64       # per sequence
# ---- what rxw_fast and express_fits branch on (csrc/grdma_engine_kernels.inc, csrc/grdma_rx_plan.hip) ----------------
RMAX = 8                # records the walk accepts ("constexpr uint32_t RMAX = 8")
REC_MAX = 512           # "hlo > 512"
T_MAX = 512             # "T > 512", EXPRESS_BYTES
EXT_BYTES = 1024        # RXW_EXT_WORDS * 8
MINRD = 256             # GRDMA_MIN_READ_SLICE
RING_MIN = 2048         # "cap < 2048"
HIST = 1024             # GRDMA_RX_HIST
# ---- the sender's unary branch (csrc/grdma_tx_body.h: "nrec_total <= 4 && __ballot(my_pay > 256) == 0") --------------
TX_UNARY_RECORDS = 4
TX_UNARY_BYTES = 256
WIRE_STAGED, WIRE_DIRECT, WIRE_FINE, WIRE_ORDERED = 0, 2, 4, 8


def enc(n):
    return 16 + ((n + 7) & ~7)


def window_bytes(ring):
    """The receive window a blocking pair arms its standing order with (op.arena_cap): one half of the pinned arena,
    grdma_pair_set_latency_mode in csrc/grdma_host_poller.inc -- 2 * ring + 4096, at most 64 MiB -- handed to the watcher
    by watch_fill_cmd (csrc/grdma_host_engine.inc: fill_rxop(p, p->h_arena, p->h_arena_cap, ...))."""
    return min(2 * ring + 4096, 64 << 20)


_CONSTS = None


def product_constants():
    """sizeof(grdma_tx_op) in words, GRDMA_FAST_WORDS, GRDMA_CMD_MAX_SGES, GRDMA_CMD_INLINE_BYTES: from the product's
    own header through the host compiler (nothing of it is restated here)."""
    global _CONSTS
    if _CONSTS is None:
        hdrs = [os.path.join(CSRC, "grdma_ops.h"), os.path.join(CSRC, "grdma_dev.h")]
        out_dir = os.path.join(ROOT, "oracle", "_build")
        os.makedirs(out_dir, exist_ok=True)
        cache = os.path.join(out_dir, "latency_sweep_consts.txt")
        if not os.path.exists(cache) or any(os.path.getmtime(h) > os.path.getmtime(cache) for h in hdrs):
            with tempfile.TemporaryDirectory(dir=out_dir) as td:
                src, exe = os.path.join(td, "c.cc"), os.path.join(td, "c")
                with open(src, "w") as f:
                    f.write('#include <stdio.h>\n#include "grdma_ops.h"\nint main() { printf("%zu %d %d %d\\n", '
                            'sizeof(grdma_tx_op) / 8, GRDMA_FAST_WORDS, GRDMA_CMD_MAX_SGES, GRDMA_CMD_INLINE_BYTES); return 0; }\n')
                subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I" + CSRC, src, "-o", exe])
                text = subprocess.check_output([exe], text=True)
                tmp = os.path.join(td, "out")
                with open(tmp, "w") as f:
                    f.write(text)
                os.replace(tmp, cache)
        with open(cache) as f:
            opw, fast_words, max_sges, inline_bytes = (int(x) for x in f.read().split())
        _CONSTS = dict(opw=opw, fast_words=fast_words, max_sges=max_sges, inline_bytes=inline_bytes)
    return _CONSTS


def fast_lane_words(sizes):
    """Words a Send of these slices takes in the mailbox's fast lane (pack_fast, csrc/grdma_host_engine.inc):
    header word + op + slice table + payload."""
    return 1 + product_constants()["opw"] + 2 * len(sizes) + (sum(sizes) + 7) // 8


def fast_lane_fit(nslices, words):
    """The largest payload of `nslices` slices whose command takes exactly `words` fast-lane words."""
    return 8 * (words - 1 - product_constants()["opw"] - 2 * nslices)


# ----------------------------------------------------------------------------------------------------------------------
# The predicate: does the watcher's single-wave drain take this drain?  Restated from rxw_fast (guards in the order of
# the source) and express_fits; everything it is given comes from the oracle.
# ----------------------------------------------------------------------------------------------------------------------
def express_fits(leftover0, n0, T, max_slices, arena_cap, rem1, credit_due):
    """-> (0 | 1 | 2, the arena clause was what declined)"""
    if T > T_MAX or max_slices < 1:
        return 0, False
    alloc = leftover0 if leftover0 else max(n0, MINRD)
    if T <= alloc:
        next_alloc = (alloc - T) or MINRD
        ok = alloc <= arena_cap and ((T + 15) & ~15) + next_alloc <= arena_cap
        return (1, False) if ok else (0, True)
    if leftover0 == 0 or max_slices < 2 or credit_due:
        return 0, False
    rest, alloc2 = T - leftover0, max(rem1, MINRD)
    if rest > alloc2:
        return 0, False
    off1 = (leftover0 + 15) & ~15
    off2 = (off1 + rest + 15) & ~15
    alloc3 = (alloc2 - rest) or MINRD
    ok = off1 + alloc2 <= arena_cap and off2 + alloc3 <= arena_cap
    return (2, False) if ok else (0, True)


def predict(cap, flags, max_reads, head, remain, irs, leftover, recs):
    """One drain over the records `recs` (payload sizes, the whole of [head, wire_tail)) -> dict: taken, reason, and
    what the witnesses ask about."""
    E = sum(enc(n) for n in recs)
    T = sum(recs)
    d = dict(cap=cap, head=head, irs=irs, leftover=leftover, recs=list(recs), E=E, T=T, words=E // 8, v=len(recs),
             taken=False, reason=None, fits=0, split=False, rem1=0, credit_due=irs + E >= cap // 2)
    # the credit rule, record by record (what either drain must do): the record that crosses ring / 2
    d["credit_rec"], d["credit_exact"], d["credit_head"], d["credit_past_end"] = None, False, None, False
    d["max_reads"] = max_reads
    run, xe = irs, 0
    for r, n in enumerate(recs):
        run += enc(n)
        xe += enc(n)
        if run >= cap // 2:
            if d["credit_rec"] is None:
                d["credit_rec"], d["credit_exact"] = r, run == cap // 2
            d["credit_head"], d["credit_past_end"] = (head + xe) & (cap - 1), head + xe >= cap
            run = 0
    # where the ring's end falls in the extent: bytes of the record in front of the end
    d["wrap"] = None
    if head + E == cap:
        d["wrap"] = "new_head_0"
    elif head + E > cap:
        x = 0
        for n in recs:
            o = cap - head - x
            if 0 <= o < enc(n):
                d["wrap"] = "between" if o == 0 else "header" if o == 8 else "footer" if o == enc(n) - 8 else "payload"
                break
            x += enc(n)
    if flags & WIRE_ORDERED:
        d["reason"] = "ordered_wire"        # !S0.limited
    elif remain != 0:
        d["reason"] = "remain"
    elif E == 0 or E > EXT_BYTES:
        d["reason"] = "extent"
    elif cap < RING_MIN:
        d["reason"] = "small_ring"
    elif max_reads < 1:
        d["reason"] = "max_reads"
    elif len(recs) > RMAX:
        d["reason"] = "records"              # the walk ends with pos != E
    elif any(n > REC_MAX for n in recs):
        d["reason"] = "record_size"
    elif T > T_MAX:
        d["reason"] = "message_size"
    else:
        rem1 = 0
        if leftover != 0 and leftover < T:
            x = 0
            for n in recs:
                if x <= leftover < x + n:
                    rem1 = x + n - leftover
                x += n
        fits, arena = express_fits(leftover, recs[0], T, min(max_reads, 8192), window_bytes(cap), rem1, d["credit_due"])
        assert not arena, "the arena clause of express_fits never binds for T <= 512"
        d["rem1"], d["fits"], d["split"] = rem1, fits, fits == 2
        if fits == 0:
            alloc = leftover if leftover else max(recs[0], MINRD)
            d["reason"] = ("no_open_read" if leftover == 0 else "max_reads" if max_reads < 2 else
                           "credit_in_split" if d["credit_due"] else "rest_over_alloc2") if T > alloc else "fits"
        else:
            d["taken"] = True
    return d


# ----------------------------------------------------------------------------------------------------------------------
# Builder and reference
# ----------------------------------------------------------------------------------------------------------------------
CONT = "continue the cut write"


class Seq:
    """One sequence of messages a -> b with its oracle trace.  Lockstep (default): a message, then its drain(s), taken
    at once.  Deferred (`groups`): a completion is left untaken while the next group is written, so that the watcher
    drains the whole group in one pass when the completion is taken; the first group primes this with one message."""

    def __init__(self, ring, flags=WIRE_STAGED, max_reads=64, deferred=False):
        self.ring, self.flags, self.max_reads, self.deferred = ring, flags, max_reads, deferred
        self.o = pyorc.OracleLink(ring, MAX_SGE)
        self.steps, self.drains, self.sends = [], [], []
        self.pending, self.eaten = [], 0      # records in b's ring (payload sizes) / bytes of the first already read
        self.hist = []                        # encoded size of every record, in order
        self.nmsg = 0
        self.cut = None                       # (slices, index, byte index) of a write the free space cut
        self.final = None

    # -- state in front of the next message (everything before it has been drained)
    @property
    def head(self):
        return self.o.state(1)["head"]

    @property
    def irs(self):
        return self.o.state(1)["internal_read_size"]

    @property
    def leftover(self):
        return int(self.o.p[1].leftover_cap)

    def _payload(self, recs):
        k = self.nmsg
        return [bytes((k * 29 + r * 13 + i * 7 + 1) % 251 for i in range(n)) for r, n in enumerate(recs)]

    def msg(self, recs):
        return self.group([recs])

    def group(self, msgs, cut=False):
        assert self.final is None
        step = dict(writes=[], drains=[])
        if self.deferred and not self.steps:
            assert len(msgs) == 1, "a deferred sequence is primed with one message"
        for i, recs in enumerate(msgs):
            st0 = self.o.state(0)
            if recs is CONT:
                assert i == 0 and self.cut is not None
                sl, idx, bidx = self.cut
                sent = self.o.send(0, sl[idx:], bidx)
                assert sent == sum(len(x) for x in sl[idx:]) - bidx, "the continuation goes out whole"
                step["writes"].append(("cont", None, [sent], True))
                made = [len(sl[idx]) - bidx] + [len(x) for x in sl[idx + 1:]]
                self.cut = None
            else:
                assert self.cut is None and 1 <= len(recs) <= MAX_SGE and min(recs) >= 1
                self.nmsg += 1
                assert self.nmsg <= MAX_MESSAGES
                sl = self._payload(recs)
                total = sum(recs)
                sent = self.o.send(0, sl)
                if cut and i == len(msgs) - 1:
                    assert self.deferred and 0 < sent < total, ("the free space cuts this Send", sent, total)
                    idx, left, made = 0, sent, []
                    while left >= len(sl[idx]):
                        left -= len(sl[idx])
                        made.append(len(sl[idx]))
                        idx += 1
                    if left:
                        made.append(left)
                    assert self.o.send(0, sl[idx:], left) == 0, "no room for more while the completion is untaken"
                    self.cut = (sl, idx, left)
                    step["writes"].append(("write", sl, [sent, 0], False))
                else:
                    assert sent == total, ("one Send takes the message whole", recs, sent)
                    step["writes"].append(("write", sl, [sent], True))
                    made = list(recs)
            self.sends.append(dict(tail0=st0["remote_tail"], recs=made, offered=None if recs is CONT else list(recs),
                                   cap=self.ring, cut=bool(cut and i == len(msgs) - 1),
                                   staged=sum(enc(n) for n in made)))
            self.pending += made
            self.hist += [enc(n) for n in made]
        while self.o.readable(1):
            step["drains"].append(self._drain())
            if self.deferred:
                assert not self.o.readable(1), "a group is one drain"
        assert step["drains"]
        self.steps.append(step)
        return step["drains"][-1]

    def _drain(self):
        st = self.o.state(1)
        assert (st["remain"] != 0) == (self.eaten != 0)
        d = predict(self.ring, self.flags, self.max_reads, st["head"], st["remain"], st["internal_read_size"],
                    self.leftover, self.pending)
        reads, wb = [], False
        while len(reads) < self.max_reads:
            got, _alloc = self.o.endpoint_read(1)
            if not got:
                wb = True
                break
            reads.append(got)
        d["reads"], d["would_block"], d["index"] = reads, wb, len(self.drains)
        n = sum(len(x) for x in reads) + self.eaten
        while self.pending and n >= self.pending[0]:
            n -= self.pending.pop(0)
        self.eaten = n
        if d["taken"]:   # the single-wave drain always empties the extent: one read, or the split's two
            assert not self.pending and len(reads) == (2 if d["split"] else 1)
        self.drains.append(d)
        return d

    # -- steering, with single-record messages
    def _advance(self, dist, filler):
        """Messages whose encoded sizes add up to `dist` (a multiple of 8), the last one a record of at most 256 bytes.
        With the default filler of 256 bytes the open read is filled exactly first: every filler then is one read of a
        fresh 256, never a split, and the credit counter only ever resets at the end of a record."""
        assert dist % 8 == 0 and (dist == 0 or dist >= 24), dist
        L = self.leftover
        if filler == MINRD and 0 < L < MINRD and dist - enc(L) > 16 + TX_UNARY_BYTES:
            self.msg([L])
            dist -= enc(L)
        while dist > 16 + TX_UNARY_BYTES:
            f = filler if dist - enc(filler) >= 24 else 112
            self.msg([f])
            dist -= enc(f)
        if dist:
            self.msg([dist - 16])

    def ready(self, L, recs):
        """An open read of L bytes in front of a drain of `recs` that does not reach the credit threshold: the steps that
        move the credit counter on ([L] fills the read exactly, [256 - L] opens it again) leave L as it is."""
        self.to_leftover(L)
        while self.irs + sum(enc(n) for n in recs) >= self.ring // 2:
            self.msg([L])
            if L < MINRD:
                self.msg([MINRD - L])
        assert self.leftover == L
        return self

    def to_head(self, target, filler=MINRD):
        dist = (target - self.head) % self.ring
        if 0 < dist < 24:
            dist += self.ring       # (less than the smallest record: a lap of the ring more)
        self._advance(dist, filler)
        assert self.head == target % self.ring
        return self

    def to_head_open(self, target, need, filler=MINRD):
        """Head at `target` with an open read of at least `need` bytes, so that the next drain is one read.  The last
        steps are laid out from the open read they meet: [leftover] fills it (a fresh 256 is next), records of one
        byte and one adjusting record cover the rest of the way with less than 256 - need bytes of payload."""
        assert need <= 128
        self.to_head(target - 320, filler)
        self.msg([self.leftover])
        r = (target - self.head) % self.ring
        while r > 16 + (MINRD - need) - 8:
            self.msg([1])
            r -= enc(1)
        self.msg([r - 16])
        assert self.head == target % self.ring and self.leftover >= need
        return self

    def to_irs(self, target):
        """internal_read_size at `target` in front of the next message.  (A credit that falls into a split is posted
        between the two reads, inside a record: the counter is then no multiple of 8 until the next credit.)"""
        assert target % 8 == 0 and (target == 0 or 24 <= target < self.ring // 2)
        while self.irs > target or self.irs % 8 or 0 < target - self.irs < 24:
            self.msg([self.leftover if 0 < self.leftover < MINRD else MINRD])
        self._advance(target - self.irs, MINRD)
        assert self.irs == target
        return self

    def to_leftover(self, want):
        """An open read with `want` bytes of room in front of the next message."""
        assert 1 <= want <= MINRD
        for _ in range(8):
            L = self.leftover
            if L == want:
                return self
            room = L if L else MINRD        # (no read open: the next one is a fresh 256 for a record of at most 256)
            if room > want:
                self.msg([min(room - want, TX_UNARY_BYTES)])
            else:
                self.msg([room])            # exactly the open read: a fresh one is next
        raise AssertionError(("leftover", self.leftover, want))

    def finish(self):
        assert self.cut is None and not self.pending and self.eaten == 0
        o = self.o
        hist = [0] * HIST
        for i, e in enumerate(self.hist):
            hist[i % HIST] = e
        self.final = dict(state=(o.state(0), o.state(1)), leftover=int(o.p[1].leftover_cap),
                          rings=(o.ring_mem(0), o.ring_mem(1)), hist=hist, hist_count=len(self.hist),
                          predicted=sum(1 for d in self.drains if d["taken"]))
        o.close()
        self.o = None
        return self


# ----------------------------------------------------------------------------------------------------------------------
# Replay on the device
# ----------------------------------------------------------------------------------------------------------------------
def _wait_ready(p, timeout=20.0):
    t0 = time.time()
    while not p.armed_ready():
        assert time.time() - t0 < timeout, "the watcher never delivered"


def run_on_device(g, seq, fast, count_exact=True):
    """The sequence on a connection a -> b whose reads a watcher of the latency engine carries out; every drain's reads
    against the oracle's, then counters, state, rings and b's record-size history.  `fast`: GRDMA_WATCH_FAST as the
    caller has set it (read when the engine starts)."""
    lib = g.load()
    F = seq.final
    a, b = mk_link(g, seq.ring, MAX_SGE, seq.flags)
    a.set_latency_mode(True)
    b.set_latency_mode(True)
    b.arm_read(seq.max_reads)
    # (the counters are copied from device symbols: read while no engine is resident)
    fd0, xd0 = int(lib.grdma_watch_fast_drains()), int(lib.grdma_express_drains())
    taken = 0

    def read():
        """Pair.endpoint_read, and where the reads lie in the window"""
        arr = (g._lib.ReadSlice * seq.max_reads)()
        wb = C.c_int(0)
        n = g._lib.check(lib.grdma_endpoint_read(b.h, seq.max_reads, arr, seq.max_reads, C.byref(wb)))
        out = []
        for i in range(n):
            dst = C.create_string_buffer(max(1, arr[i].len))
            g._lib.check(lib.grdma_pair_arena_copy_out(b.h, arr[i].off, dst, arr[i].len))
            out.append(dst.raw[:arr[i].len])
        return (out, bool(wb.value)), [(int(arr[i].off), int(arr[i].len)) for i in range(n)]

    def take(d):
        got, offs = read()
        # (packed: each read at the 16-byte boundary behind the one before)
        assert all(o % 16 == 0 and o - offs[0][0] == sum((n + 15) & ~15 for _, n in offs[:i]) for i, (o, _) in enumerate(offs)), \
            ("drain", d["index"], offs)
        assert got == (d["reads"], d["would_block"]), ("drain", d["index"], d["recs"], d["reason"], [len(x) for x in got[0]],
                                                      got[1], [len(x) for x in d["reads"]], d["would_block"])

    def write(w):
        kind, sl, steps, done = w
        got = a.endpoint_write(sl) if kind == "write" else a.endpoint_write_continue()
        assert got == (steps, done), (kind, got, steps, done)
    g._lib.check(lib.grdma_engine_start())
    try:
        untaken = None
        for step in seq.steps:
            for w in step["writes"]:
                write(w)
            if seq.deferred:
                if untaken is not None:
                    take(untaken)      # (copied out while the drain it lets go writes the other window)
                    taken += 1
                _wait_ready(b)
                untaken = step["drains"][0]
            else:
                for d in step["drains"]:
                    _wait_ready(b)
                    take(d)
                    taken += 1
        if untaken is not None:
            take(untaken)
            taken += 1
        assert b.endpoint_read(seq.max_reads) == ([], True)    # nothing behind the last drain
        assert b.watch_hits() == taken == len(seq.drains)
    finally:
        lib.grdma_engine_stop()
    fd, xd = int(lib.grdma_watch_fast_drains()) - fd0, int(lib.grdma_express_drains()) - xd0
    want = F["predicted"] if fast else 0
    if count_exact or not fast:
        assert fd == want, ("single-wave drains", fd, "predicted", want,
                            [(d["index"], d["recs"], d["reason"]) for d in seq.drains if not d["taken"]][:8])
    assert xd >= fd
    sa, sb = a.state(), b.state()
    for k in STATE_KEYS:
        assert sa[k] == F["state"][0][k], ("a", k, sa[k], F["state"][0][k])
        assert sb[k] == F["state"][1][k], ("b", k, sb[k], F["state"][1][k])
    assert sb["leftover_cap"] == F["leftover"]
    assert a.ring_mem() == F["rings"][0] and b.ring_mem() == F["rings"][1]
    h = (C.c_uint32 * 4096)()
    cnt, per = C.c_uint64(), C.c_uint32()
    assert lib.grdma_pair_debug_hist(b.h, h, C.byref(cnt), C.byref(per)) == 0
    assert int(cnt.value) == F["hist_count"]
    got_hist = [int(x) for x in h[:HIST]]
    assert got_hist == F["hist"], [(i, x, y) for i, (x, y) in enumerate(zip(got_hist, F["hist"])) if x != y][:8]
    assert lib.grdma_pair_debug_hist(a.h, h, C.byref(cnt), C.byref(per)) == 0 and int(cnt.value) == 0
    a.close()
    b.close()


# ----------------------------------------------------------------------------------------------------------------------
# The cases.  A case is a function that builds a Seq from the constants above and the witnesses it needs: (label,
# predicate over the finished Seq).  No random draws.
# ----------------------------------------------------------------------------------------------------------------------
CASES = []   # dict(id, fam, build, needs, exact: the drain count is asserted, seq: the finished Seq)


def case(fam, name, needs, exact=True):
    def reg(fn):
        CASES.append(dict(id="%s-%s" % (fam, name), fam=fam, build=fn, needs=needs, exact=exact, seq=None))
        return fn
    return reg


def some(label, fn):
    """some drain satisfies fn"""
    return (label, lambda s: any(fn(d) for d in s.drains))


def some_send(label, fn):
    return (label, lambda s: any(fn(x) for x in s.sends))


def took(fn):
    return lambda d: d["taken"] and fn(d)


def declined(reason, fn=lambda d: True):
    return lambda d: not d["taken"] and d["reason"] == reason and fn(d)


WIRES = {WIRE_STAGED: "staged", WIRE_DIRECT: "direct", WIRE_FINE: "finegrained"}


# ---- A: the limits of one drain --------------------------------------------------------------------------------------
for _ring, _fl in ((2048, WIRE_STAGED), (4096, WIRE_DIRECT), (65536, WIRE_FINE)):
    @case("A", "message_511_512_513_r%d_%s" % (_ring, WIRES[_fl]),
          [some("one record of 511 taken", took(lambda d: d["recs"] == [511])),
           some("one record of 512 taken", took(lambda d: d["recs"] == [512])),
           some("one record of 513 declined", declined("record_size", lambda d: d["recs"] == [513])),
           some("255 + 256 taken", took(lambda d: d["recs"] == [255, 256])),
           some("256 + 256 taken", took(lambda d: d["recs"] == [256, 256])),
           some("256 + 257 declined", declined("message_size", lambda d: d["recs"] == [256, 257]))])
    def _a_t(ring=_ring, fl=_fl):
        s = Seq(ring, fl)
        for recs in ([511], [512], [513], [255, 256], [256, 256], [256, 257]):
            s.ready(MINRD, recs).msg(recs)
        return s

_R8, _R9, _R512 = [56] * 8, [56] * 9, [65] * 7 + [57]
for _ring, _fl in ((4096, WIRE_FINE), (2048, WIRE_DIRECT)):
    @case("A", "records_8_9_one_message_r%d_%s" % (_ring, WIRES[_fl]),
          [some("8 records taken", took(lambda d: d["recs"] == _R8)),
           some("9 records declined", declined("records", lambda d: d["recs"] == _R9)),
           some("8 records, T = 512, 87 words taken", took(lambda d: d["recs"] == _R512 and d["T"] == 512 and d["words"] == 87))])
    def _a_rec(ring=_ring, fl=_fl):
        s = Seq(ring, fl)
        for recs in (_R8, _R9, _R512, _R8):
            s.ready(MINRD, recs).msg(recs)
        return s

    @case("A", "records_8_9_as_groups_r%d_%s" % (_ring, WIRES[_fl]),
          [some("8 messages in one drain taken", took(lambda d: d["recs"] == _R8)),
           some("9 messages in one drain declined", declined("records", lambda d: d["recs"] == _R9)),
           some("8 messages, T = 512 taken", took(lambda d: d["recs"] == _R512))])
    def _a_grp(ring=_ring, fl=_fl):
        s = Seq(ring, fl, deferred=True)
        s.msg([40])
        for recs in (_R8, _R9, _R512, _R8):
            s.ready(MINRD, recs)
            s.group([[n] for n in recs])
        return s

for _ring, _fl in ((2048, WIRE_FINE), (4096, WIRE_STAGED)):
    @case("A", "extent_words_and_tails_r%d_%s" % (_ring, WIRES[_fl]),
          [some("64 words taken", took(lambda d: d["words"] == 64)),
           some("65 words taken", took(lambda d: d["words"] == 65)),
           some("87 words taken", took(lambda d: d["words"] == 87))] +
          [some("T & 7 == %d taken, unsplit" % k, took(lambda d, k=k: d["T"] & 7 == k and not d["split"])) for k in range(8)] +
          [some("T & 7 == %d taken, split" % k, took(lambda d, k=k: d["T"] & 7 == k and d["split"])) for k in range(8)])
    def _a_words(ring=_ring, fl=_fl):
        s = Seq(ring, fl)
        for recs in ([496], [504], _R512):           # 16 + 496 = 64 words, 16 + 504 = 65 words, 87 words
            s.ready(MINRD, recs).msg(recs)
        for n in range(41, 49):                      # the tail of the last delivered word, in one read ...
            s.ready(64, [n]).msg([n])
        for n in range(41, 49):                      # ... and in the second piece of a split
            s.ready(16, [n]).msg([n])
        return s

    @case("A", "record_sizes_1_7_8_9_r%d_%s" % (_ring, WIRES[_fl]),
          [some("a record of %d alone taken" % n, took(lambda d, n=n: d["recs"] == [n])) for n in (1, 7, 8, 9)] +
          [some("1, 7, 8, 9 in one drain taken", took(lambda d: d["recs"] == [1, 7, 8, 9])),
           some("9, 8, 7, 1 in one drain taken", took(lambda d: d["recs"] == [9, 8, 7, 1]))])
    def _a_small(ring=_ring, fl=_fl):
        s = Seq(ring, fl)
        for recs in ([1], [7], [8], [9], [1, 7, 8, 9], [9, 8, 7, 1]) * 4:
            s.msg(recs)
        return s


@case("A", "ring_1024_declines", [some("declined by the ring size", declined("small_ring"))])
def _a_r1024():
    s = Seq(1024, WIRE_STAGED)
    for recs in ([40], [100], [8], [1, 7, 8, 9], [200]) * 3:
        s.msg(recs)
    assert not any(d["taken"] for d in s.drains)
    return s


# ---- B: the open read ------------------------------------------------------------------------------------------------
def _b_chain(ring, fl, Ls):
    s = Seq(ring, fl)
    for L in Ls:
        for T in (L - 1, L, L + 1):
            if T >= 1:
                s.ready(L, [T]).msg([T])
    return s


for _name, _Ls, _ring, _fl in (("L1_4", (1, 2, 3, 4), 2048, WIRE_STAGED), ("L5_8", (5, 6, 7, 8), 4096, WIRE_DIRECT),
                               ("L9_15_16_17_255", (9, 15, 16, 17, 255), 2048, WIRE_FINE)):
    @case("B", "leftover_%s_r%d_%s" % (_name, _ring, WIRES[_fl]),
          [some("leftover %d, T = L - 1 taken in one read" % L, took(lambda d, L=L: d["leftover"] == L and d["T"] == L - 1 and not d["split"]))
           for L in _Ls if L > 1] +
          [some("leftover %d, T = L taken in one read" % L, took(lambda d, L=L: d["leftover"] == L and d["T"] == L and not d["split"]))
           for L in _Ls] +
          [some("leftover %d, T = L + 1 taken as a split" % L, took(lambda d, L=L: d["leftover"] == L and d["T"] == L + 1 and d["split"]))
           for L in _Ls] +
          [("a read filled exactly leaves a fresh 256",
            lambda s: any(d["taken"] and d["T"] == d["leftover"] and s.drains[d["index"] + 1]["leftover"] == MINRD
                          for d in s.drains[:-1]))])
    def _b_L(ring=_ring, fl=_fl, Ls=_Ls):
        return _b_chain(ring, fl, Ls)

for _ring, _fl in ((4096, WIRE_FINE), (2048, WIRE_DIRECT)):
    @case("B", "split_boundaries_r%d_%s" % (_ring, WIRES[_fl]),
          [some("split with L & 7 == %d" % k, took(lambda d, k=k: d["split"] and d["leftover"] & 7 == k)) for k in range(8)] +
          [some("L on a record boundary: rem1 is the whole next record",
                took(lambda d: d["split"] and d["leftover"] == d["recs"][0] and d["rem1"] == d["recs"][1])),
           some("L inside a record", took(lambda d: d["split"] and d["v"] >= 2 and d["leftover"] < d["recs"][0])),
           some("L inside the second record", took(lambda d: d["split"] and d["v"] >= 2 and d["recs"][0] < d["leftover"] < d["recs"][0] + d["recs"][1])),
           some("rem1 above 256", took(lambda d: d["split"] and d["rem1"] > MINRD and d["recs"] == [6, 300])),
           some("rest == alloc2 taken", took(lambda d: d["split"] and d["T"] - d["leftover"] == max(d["rem1"], MINRD))),
           some("rest == alloc2 + 1 declined", declined("rest_over_alloc2", lambda d: d["T"] - d["leftover"] == max(d["rem1"], MINRD) + 1))])
    def _b_split(ring=_ring, fl=_fl):
        s = Seq(ring, fl)
        for L in range(8, 16):                               # L & 7 = 0 .. 7, a two-record message across the boundary
            recs = [L + 3, 40]
            s.ready(L, recs).msg(recs)
        for L, recs in ((6, [6, 40]), (6, [3, 40]), (6, [6, 300]), (6, [6, 100, 156]), (6, [6, 100, 157]),
                        (20, [20, 256]), (20, [20, 257]), (17, [17, 1, 300])):
            s.ready(L, recs).msg(recs)
        return s


@case("B", "no_open_read_r4096_staged",
      [some("T > 256 with no read open declined", declined("no_open_read", lambda d: d["leftover"] == 0 and d["T"] > MINRD))])
def _b_fresh():
    s = Seq(4096, WIRE_STAGED)
    s.msg([200, 100])
    for recs in ([40], [112], [8]) * 6:
        s.msg(recs)
    return s


@case("B", "first_record_300_no_open_read_r2048_direct",
      [some("a first record above 256 with no read open taken", took(lambda d: d["leftover"] == 0 and d["recs"] == [300]))])
def _b_fresh2():
    s = Seq(2048, WIRE_DIRECT)
    s.msg([300])               # (the record at the head sizes the first read: max(256, 300))
    for recs in ([40], [112], [8]) * 6:
        s.msg(recs)
    return s


# ---- C: credit -------------------------------------------------------------------------------------------------------
def _credit_pos(s, recs, at):
    """irs such that record `at` of recs lands exactly on ring / 2"""
    return s.ring // 2 - sum(enc(n) for n in recs[:at + 1])


for _ring, _fl in ((2048, WIRE_STAGED), (4096, WIRE_FINE), (2048, WIRE_DIRECT)):
    @case("C", "threshold_minus8_exact_plus8_r%d_%s" % (_ring, WIRES[_fl]),
          [some("irs + E == ring / 2 - 8: no credit", took(lambda d: d["irs"] + d["E"] == d["cap"] // 2 - 8 and d["credit_rec"] is None)),
           some("irs + E == ring / 2: credit", took(lambda d: d["irs"] + d["E"] == d["cap"] // 2 and d["credit_exact"])),
           some("irs + E == ring / 2 + 8: credit", took(lambda d: d["irs"] + d["E"] == d["cap"] // 2 + 8 and d["credit_rec"] is not None)),
           some("exact on the first of three records", took(lambda d: d["v"] == 3 and d["credit_rec"] == 0 and d["credit_exact"])),
           some("exact on the second of three records", took(lambda d: d["v"] == 3 and d["credit_rec"] == 1 and d["credit_exact"])),
           some("exact on the last of three records", took(lambda d: d["v"] == 3 and d["credit_rec"] == 2 and d["credit_exact"]))])
    def _c_thr(ring=_ring, fl=_fl):
        s = Seq(ring, fl)
        for delta in (-8, 0, 8):
            s.to_irs(ring // 2 - enc(1) + delta).msg([1])
        for at in (0, 1, 2):
            s.to_irs(_credit_pos(s, [1, 1, 1], at)).msg([1, 1, 1])
        return s

for _ring, _fl in ((2048, WIRE_FINE), (4096, WIRE_DIRECT)):
    @case("C", "split_wrap_and_plan_body_r%d_%s" % (_ring, WIRES[_fl]),
          [some("a credit due during a split declined", declined("credit_in_split")),
           some("exact equality in a drain the plan body runs", declined("record_size", lambda d: d["credit_exact"])),
           some("exact equality in a drain the plan body runs, credit not last",
                declined("records", lambda d: d["credit_exact"] and d["credit_rec"] < d["v"] - 1))])
    def _c_split(ring=_ring, fl=_fl):
        s = Seq(ring, fl)
        s.to_irs(ring // 2 - 24)
        s.msg([min(s.leftover + 1, REC_MAX)])
        s.to_irs(_credit_pos(s, [513], 0)).msg([513])
        nine = [8] * 9
        s.to_irs(_credit_pos(s, nine, 4)).msg(nine)
        return s

for _ring, _fl in ((2048, WIRE_STAGED), (4096, WIRE_DIRECT)):
    @case("C", "unary_stream_112_r%d_%s" % (_ring, WIRES[_fl]),
          [some("a taken drain whose credit counter lands exactly on ring / 2", took(lambda d: d["credit_exact"])),
           some("a taken drain whose credit head is the ring's end: 0", took(lambda d: d["credit_past_end"] and d["credit_head"] == 0))])
    def _c_stream(ring=_ring, fl=_fl):
        s = Seq(ring, fl)
        for _ in range(24 * ring // 2048):
            s.msg([112])      # (every second one of these meets an open read of 32 and is split; 112 + 16 divides ring / 2)
        return s

for _recs, _at, _ring, _fl in (([40, 40], 0, 2048, WIRE_DIRECT), ([40, 40, 40], 2, 4096, WIRE_FINE), ([40, 40, 40], 1, 2048, WIRE_STAGED)):
    @case("C", "credit_head_past_the_end_rec%d_of_%d_r%d_%s" % (_at, len(_recs), _ring, WIRES[_fl]),
          [some("record %d of %d credits and ends 8 bytes past the ring's end" % (_at, len(_recs)),
                took(lambda d, r=_recs, a=_at: d["recs"] == r and d["credit_rec"] == a and d["credit_past_end"] and d["credit_head"] == 8))])
    def _c_past(recs=_recs, at=_at, ring=_ring, fl=_fl):
        s = Seq(ring, fl)
        s.to_irs(ring // 2 - enc(1)).msg([1])       # a credit exactly at ring / 2: the counter restarts there
        # ring / 2 + 8 bytes later record `at` ends at offset 8
        s.to_head_open(ring + 8 - (at + 1) * enc(40), sum(recs)).msg(recs)
        return s


# ---- D: the ring's end ------------------------------------------------------------------------------------------------
def _d_needs(v):
    return [some("the end %s, %d record(s), taken" % (k, v), took(lambda d, k=k, v=v: d["wrap"] == k and d["v"] == v))
            for k in (("header", "payload", "footer", "new_head_0") if v == 1 else ("header", "payload", "footer", "between", "new_head_0"))]


for _ring, _fl, _filler in ((2048, WIRE_STAGED, MINRD), (2048, WIRE_DIRECT, MINRD), (4096, WIRE_FINE, 496)):
    @case("D", "one_record_r%d_%s" % (_ring, WIRES[_fl]), _d_needs(1))
    def _d_one(ring=_ring, fl=_fl, filler=_filler):
        s = Seq(ring, fl)
        for back in (8, 24, enc(40) - 8, enc(40)):       # header word last, payload, footer word first, new head 0
            s.to_head_open(ring - back, 40, filler).msg([40])
        return s

    @case("D", "three_records_r%d_%s" % (_ring, WIRES[_fl]), _d_needs(3))
    def _d_three(ring=_ring, fl=_fl, filler=_filler):
        s = Seq(ring, fl)
        recs = [9, 40, 7]                                   # 32 + 56 + 24: the end inside / around the middle record
        # bytes from the head to the ring's end: behind the middle record's header word, in its payload, in front of its
        # footer word, between the first two records, and the whole extent
        for back in (enc(9) + 8, enc(9) + 24, enc(9) + enc(40) - 8, enc(9), enc(9) + enc(40) + enc(7)):
            s.to_head_open(ring - back, sum(recs), filler).msg(recs)
        return s


# ---- E: max_reads 1, 2, 3 ----------------------------------------------------------------------------------------------
def _e_needs(mr):
    need = [some("one read, taken", took(lambda d: d["fits"] == 1)),
            some("a drain that ends inside a record", lambda d: d["index"] >= 0 and d.get("left_remain")),
            some("a drain behind one that ended inside a record declined", declined("remain"))] if mr < 3 else \
           [some("one read, taken", took(lambda d: d["fits"] == 1)),
            some("three reads in one drain", lambda d: len(d["reads"]) == 3 and not d["taken"])]
    if mr == 1:
        need += [some("a split declined at max_reads 1", declined("max_reads", lambda d: d["leftover"] and d["T"] > d["leftover"])),
                 some("the read filled exactly: no would-block read, nothing left open",
                      took(lambda d: d["T"] == (d["leftover"] or MINRD) and not d["would_block"])),
                 some("no read open in front of a taken drain", took(lambda d: d["leftover"] == 0 and d["index"] > 0))]
    else:
        need += [some("a split taken", took(lambda d: d["split"]))]
    if mr == 2:
        need += [some("a split whose second read is filled exactly: nothing left open",
                      took(lambda d: d["split"] and d["T"] - d["leftover"] == max(d["rem1"], MINRD) and not d["would_block"]))]
    return need


for _mr, _ring, _fl in ((1, 2048, WIRE_STAGED), (2, 4096, WIRE_DIRECT), (3, 2048, WIRE_FINE), (2, 2048, WIRE_STAGED), (1, 4096, WIRE_FINE)):
    @case("E", "max_reads_%d_r%d_%s" % (_mr, _ring, WIRES[_fl]), _e_needs(_mr))
    def _e(mr=_mr, ring=_ring, fl=_fl):
        s = Seq(ring, fl, max_reads=mr)
        s.msg([40])
        for L, recs in ((10, [5, 300, 20]), (64, [40]), (6, [6, 100, 156]), (20, [21]), (30, [30]), (12, [12, 256]),
                        (10, [5, 100, 300])):
            s.ready(L, recs).msg(recs)
            s.msg([7])
        s.msg([256]); s.msg([8])
        for d, nxt in zip(s.drains, s.drains[1:]):
            d["left_remain"] = nxt["reason"] == "remain"
        return s


# ---- F: the send side (parity; the receiver's count is still exact) ----------------------------------------------------
def _spread(total, n):
    """`total` bytes over n slices, as even as they go"""
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


def _f_lane_msgs():
    out = []
    for n in (1, 2, 4, 16):
        full = fast_lane_fit(n, product_constants()["fast_words"])
        out += [_spread(full - 8, n), _spread(full, n), _spread(full + 1, n)]
    return out


def _unary(x):
    return len(x["recs"]) <= TX_UNARY_RECORDS and max(x["recs"]) <= TX_UNARY_BYTES


for _ring, _fl in ((4096, WIRE_STAGED), (65536, WIRE_DIRECT), (4096, WIRE_FINE)):
    @case("F", "fast_lane_words_r%d_%s" % (_ring, WIRES[_fl]),
          [some_send("%d slices in %d words" % (n, w), lambda x, n=n, w=w: len(x["recs"]) == n and fast_lane_words(x["recs"]) == w)
           for n in (1, 2, 4, 16) for w in (55, 56, 57)] +
          [some_send("328 / 329 bytes in one slice", lambda x: x["recs"] == [329]),
           some_send("88 bytes in sixteen", lambda x: len(x["recs"]) == 16 and sum(x["recs"]) == 88)])
    def _f_lane(ring=_ring, fl=_fl):
        assert product_constants()["fast_words"] == 56 and fast_lane_fit(1, 56) == 328 and fast_lane_fit(16, 56) == 88
        s = Seq(ring, fl)
        for recs in _f_lane_msgs() * 2:
            s.msg(recs)
        return s

    @case("F", "sges_inline_bytes_records_r%d_%s" % (_ring, WIRES[_fl]),
          [some_send("16 slices", lambda x: len(x["recs"]) == 16), some_send("17 slices", lambda x: len(x["recs"]) == 17),
           some_send("1024 inline bytes", lambda x: sum(x["recs"]) == 1024 and len(x["recs"]) == 8),
           some_send("1025 inline bytes", lambda x: sum(x["recs"]) == 1025 and len(x["recs"]) == 8),
           some_send("4 records", lambda x: x["recs"] == [8] * 4), some_send("5 records", lambda x: x["recs"] == [8] * 5),
           some_send("a record of 256", lambda x: x["recs"] == [256]), some_send("a record of 257", lambda x: x["recs"] == [257]),
           some_send("4 x 256: 136 words", lambda x: x["recs"] == [256] * 4 and x["staged"] == 136 * 8),
           some_send("records of 1 and 8", lambda x: x["recs"] == [1, 8, 1, 8]),
           some_send("the unary branch writes across the ring's end",
                     lambda x: x["cap"] > 4096 or (x["recs"] == [1, 256, 256, 8] and x["tail0"] + x["staged"] > x["cap"]))])
    def _f_lim(ring=_ring, fl=_fl):
        s = Seq(ring, fl)
        for recs in ([8] * 16, [8] * 17, [128] * 8, [128] * 7 + [129], [8] * 4, [8] * 5, [256], [257], [256] * 4,
                     [1], [8], [1, 8, 1, 8]) * (2 if ring <= 4096 else 1):
            s.msg(recs)
        if ring <= 4096:
            s.to_head(ring - 24 - enc(256)).msg([1, 256, 256, 8])
        return s


@case("F", "send_cut_by_the_free_space_r2048_staged",
      [some_send("a Send the free space cuts inside the unary branch",
                 lambda x: x["cut"] and _unary(x) and sum(x["recs"]) < sum(x["offered"])),
       some_send("its continuation", lambda x: x["offered"] is None)], exact=False)
def _f_cut():
    s = Seq(2048, WIRE_STAGED, deferred=True)
    s.msg([40])
    s.to_irs(760)
    # 760 bytes not yet credited + 432 un-drained: three records of the 864 offered fit, the fourth is cut to 192 bytes
    s.group([[200, 200], [200, 200, 200, 200]], cut=True)
    s.group([CONT, [40]])
    s.msg([112])
    # (what cut it is the free space, not the staging budget: behind three records ring / 2 still has room for the fourth)
    assert pyorc.lib().orc_calc_writable(2048 // 2 - 3 * enc(200)) >= 200
    return s


# ---- G: the ordered wire (the watcher finds records by their tags; never the single-wave drain) -----------------------
_G_WRAPS = {"header": (40, 8), "payload": (255, 24), "footer": (248, enc(248) - 8), "new_head_0": (256, enc(256)), "header of 1": (1, 8)}
for _ring, _kinds in ((2048, ("header", "payload", "footer", "new_head_0", "header of 1")), (4096, ("footer", "new_head_0", "header of 1"))):
    @case("G", "ordered_wire_single_records_r%d" % _ring,
          [some("a record of %d" % n, declined("ordered_wire", lambda d, n=n: d["recs"] == [n])) for n in (1, 7, 8, 9, 248, 255, 256)] +
          [some("the end: %s" % k, declined("ordered_wire", lambda d, k=k: d["wrap"] == k.split()[0] and d["recs"] == [_G_WRAPS[k][0]]))
           for k in _kinds])
    def _g(ring=_ring, kinds=_kinds):
        s = Seq(ring, WIRE_ORDERED)
        for n in (1, 7, 8, 9, 248, 255, 256):
            s.msg([n])
        for k in kinds:
            n, back = _G_WRAPS[k]
            s.to_head(ring - back).msg([n])
        assert all(len(x["recs"]) == 1 and x["recs"][0] <= TX_UNARY_BYTES for x in s.sends)
        return s


def check_cases():
    """Build every case on the oracle and check its witnesses and the caps every sequence obeys."""
    for c in CASES:
        s = c["build"]().finish()
        c["seq"] = s
        missing = [label for label, fn in c["needs"] if not fn(s)]
        assert not missing, (c["id"], "misses its edge", missing)
        assert s.nmsg <= MAX_MESSAGES and len(s.hist) == sum(len(x["recs"]) for x in s.sends)
        if c["fam"] in "ABCD" and s.ring >= RING_MIN:
            assert 2 * s.final["predicted"] >= len(s.drains), (c["id"], "taken", s.final["predicted"], "of", len(s.drains))
    assert len(set(c["id"] for c in CASES)) == len(CASES)
    return CASES
