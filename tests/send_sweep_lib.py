"""TEST INFRASTRUCTURE: the general Send planners swept over slice lists built from their own edges.

tx_plan_body (csrc/grdma_tx_body.h, k_tx_plan: every blocking grdma_pair_send / grdma_endpoint_write_step, and in
latency mode every Send above 64 slices or 64 KiB) and tx_burst_wave (k_tx_plan_seq: up to sixteen Sends of an
asynchronous endpoint on one wavefront) branch on a handful of constants: 256 threads and the run length
per = ceil(m / 256), the pricing window guess = last + last / 4 + 64, the LDS padding of one slot per 16, the list's
end, the payload clamp at 2 * ring, the record that crosses the ring's end on a direct wire, 64 lanes and sixteen Sends
a burst.  Every case here puts the first short record, the wrapping record or the list's end at one of those indices.
Nothing is sampled at random.

`Script` is builder and reference in one (as latency_sweep_lib.Seq): every call runs `pyorc.OracleLink` at once and
records what the product has to show after the same call -- accepted bytes, last_wrs, ring image, staging image,
state of both sides, GetWritableSize, delivered reads -- so the steering helpers read tail, head and room from the
oracle itself.  `run_on_device` replays a finished Script on a connected product pair a -> b.

WITNESSES.  `price` restates the pricing rule in plain Python from the header comment of tx_plan_body and
pair.cc:660-709, fed oracle state only (the sender's remote_tail and remote_head, the slice lengths, byte_idx, the
previous Send's record count).  Its `sent` must equal the oracle's on every Send of every case, which pins it.  From it
come, per Send: m, the first short record fs, which budget bound it, short_pay, the encoded total, the record that
holds the ring's end and where in it the end falls, guess and the finally priced window.  A case names the witnesses
it needs; `check_witnesses` raises when one is missing.  On the device a non-latency Send leaves the priced window in
tx_dbg[7]: every blocking non-latency Send of the sweep asserts it against the restatement's.

Everything in the ring is a multiple of 8 bytes from the ring's start (tail, header, padded payload, footer), so the
ring's end can only fall on a word boundary of a record: behind the header word, n words into the payload, in front
of the last payload word, behind the padded payload (the footer lands at offset 0), behind the footer.

Only tests/ may import this module."""
import ctypes as C
import time
import zlib

from oracle import pyorc
from tests.pair_lib import _mask_pads, _ring_eq, check_state, mk_link

RESERVED = 24           # ring_buffer.h:52
THREADS = 256           # PLAN_THREADS
MAX_RECORDS = 4095      # GRDMA_TX_MAX_RECORDS - 1
TILE = 8192             # 1 << GRDMA_PLAN_TILE_SHIFT(ring) for rings below 32 MiB
BURST_MAX = 16          # Sends one launch of k_tx_plan_seq prices (kBurstMax)
SMALL_WAVE_BYTES = 64 << 10   # tx_plan_body's guard in front of tx_small_wave (latency mode): <= 64 slices, <= 64 KiB
WIRE_STAGED, WIRE_DIRECT = 0, 2
WIRES = {"staged": WIRE_STAGED, "direct": WIRE_DIRECT}
ERR_CAPACITY = 5
MEM_DEVICE = 0
K16, K64, K256 = 16 << 10, 64 << 10, 256 << 10


def enc(n):
    return 16 + ((n + 7) & ~7)


def W(space):
    """CalcWritableSize, ring_buffer.h:185-189"""
    return (space - RESERVED) & ~7 if space > RESERVED else 0


_BASES = {}


def fill(n, k):
    """n non-zero bytes that depend on the position in the slice and on the slice's index."""
    k %= 61
    base = _BASES.get(k)
    if base is None or len(base) < n:
        base = _BASES[k] = bytes(1 + (i * 7 + (i >> 4) * 13 + k * 29) % 255 for i in range(max(n, 4200)))
    return base[:n]


# ----------------------------------------------------------------------------------------------------------------------
# The restatement of the pricing rule
# ----------------------------------------------------------------------------------------------------------------------
def price(R, max_sge, tail, rhead, lens, byte_idx, last_records, connected=True):
    """One Send -> its witnesses.  pay_i = min(len_i, W(S - st_i), W(free0 - st_i)); the first record that comes up short
    (or is empty) ends the Send; a short payload above zero goes out as the last record."""
    S = R // 2
    free0 = R - ((tail - rhead) % R)
    m_full = min(len(lens), max_sge, MAX_RECORDS) if connected else 0
    st, recs, starts, fs, short_pay, zero = 0, [], [], None, 0, False
    for i in range(m_full):
        l = max(0, lens[i] - byte_idx) if i == 0 else lens[i]
        pay = min(l, W(S - st), W(free0 - st))
        if pay < l or l == 0:
            fs, short_pay, zero = i, pay, l == 0
            break
        starts.append(st)
        recs.append(l)
        st += enc(l)
    whole = len(recs)
    if short_pay:
        starts.append(st)
        recs.append(short_pay)
        st += enc(short_pay)
    w = dict(R=R, m=m_full, fs=fs, short_pay=short_pay, zero=zero, whole=whole, recs=recs, staged=st, sent=sum(recs),
             tail0=tail, free0=free0, bound=None, prev=last_records, byte_idx=byte_idx, offered=len(lens))
    if fs is not None and not zero:
        w["bound"] = "staging" if S < free0 else ("credit" if free0 < S else "equal")
    # the pricing window
    guess = last_records + last_records // 4 + 64
    w["guess"] = guess
    w["window"] = guess if guess < m_full and fs is not None and fs < guess else m_full
    w["repriced"] = guess < m_full and w["window"] == m_full
    w["per"] = (w["window"] + THREADS - 1) // THREADS
    # the ring's end
    u = R - tail
    w["end_rec"], w["end_at"] = None, set()
    if st and u == st:
        w["end_rec"], w["end_at"] = len(recs) - 1, {"behind_last"}
    elif u < st:
        for i, (x, p) in enumerate(zip(starts, recs)):
            e = enc(p)
            d = u - x
            if d == 0:
                w["end_rec"], w["end_at"] = i, {"between"}
                break
            if d < e:
                w["end_rec"] = i
                at = set()
                if d == 8:
                    at.add("header")
                elif d == e - 8:
                    at.add("behind_payload")
                else:
                    at.add("payload")
                    if d == 16:
                        at.add("word1")
                    if (d - 8) % TILE == 0:
                        at.add("tile")
                    if d == e - 16 and p % 8:
                        at.add("lastword")
                w["end_at"] = at
                break
    return w


# ----------------------------------------------------------------------------------------------------------------------
# Builder and reference
# ----------------------------------------------------------------------------------------------------------------------
def _z(b):
    return zlib.compress(b, 1)


class Script:
    def __init__(self, ring, max_sge, latency=False, asynchronous=False):
        self.ring, self.max_sge, self.latency, self.asynchronous = ring, max_sge, latency, asynchronous
        self.o = pyorc.OracleLink(ring, max_sge)
        self.steps, self.sends, self.bursts = [], [], []
        self.image = bytearray()      # every slice of the script, slice k at an offset of k % 16 from a 16-byte boundary
        self.nslices = 0
        self.last_records = 0         # the connection's tx_last_records in front of the next Send
        self.connected = True
        self.pads = False             # a record with a payload that is no multiple of 8 has gone out: pad bytes may differ
        self.wcur = None              # the endpoint write outstanding: [slices, views, index, byte index]
        self.final = False

    # -- oracle state
    @property
    def tail(self):
        return int(self.o.p[0].remote_tail)

    @property
    def rhead(self):
        return int(self.o.p[0].status_recv.remote_head)

    @property
    def free0(self):
        return self.ring - ((self.tail - self.rhead) % self.ring)

    @property
    def room0(self):
        return min(self.ring // 2, self.free0)

    def _mk(self, lens):
        sl, views = [], []
        for n in lens:
            k = self.nslices
            self.nslices += 1
            pos = ((len(self.image) + 15) & ~15) + k % 16
            self.image += bytes(pos - len(self.image))
            b = fill(n, k)
            self.image += b
            sl.append(b)
            views.append((pos, n))
        return sl, views

    def _snap(self, step):
        o = self.o
        step.update(ring=_z(o.ring_mem(1)), st=(o.state(0), o.state(1)), writable=int(o.writable(0)), pads=self.pads)
        self.steps.append(step)
        return step

    def _one_send(self, sl, byte_idx):
        """the oracle's Send and the restatement's, which must agree -> (sent, witness)"""
        lens = [len(x) for x in sl]
        w = price(self.ring, self.max_sge, self.tail, self.rhead, lens, byte_idx, self.last_records)
        sent = int(self.o.send(0, sl, byte_idx))
        assert sent == w["sent"], ("the restatement of the pricing rule leaves the oracle's", sent, w["sent"], w["fs"])
        assert self.tail == (w["tail0"] + w["staged"]) % self.ring
        self.last_records = len(w["recs"])
        self.pads = self.pads or any(p % 8 for p in w["recs"])
        w["index"] = len(self.sends)
        self.sends.append(w)
        return sent, w

    # -- steps
    def send(self, lens, byte_idx=0):
        """One blocking Pair.Send of a fresh slice list."""
        assert not self.final and 1 <= len(lens) <= MAX_RECORDS
        sl, views = self._mk(lens)
        if not self.connected:   # pair.cc:652-655: nothing is taken, nothing changes
            w = price(self.ring, self.max_sge, self.tail, self.rhead, lens, byte_idx, self.last_records, connected=False)
            self.last_records = 0
            w["index"] = len(self.sends)
            self.sends.append(w)
            self._snap(dict(kind="send", views=views, byte_idx=byte_idx, sent=0, wrs=None, staging=None, w=w))
            return w
        sent, w = self._one_send(sl, byte_idx)
        self._snap(dict(kind="send", views=views, byte_idx=byte_idx, sent=sent, wrs=self.o.last_wrs(0),
                        staging=_z(self.o.staging_mem(0)), w=w))
        return w

    def refused(self, count):
        """A slice list above what one plan prices: GRDMA_ERR_CAPACITY, nothing changes."""
        _sl, views = self._mk([1] * count)
        self._snap(dict(kind="refused", views=views))

    def drain(self):
        reads = []
        while True:
            got, _alloc = self.o.endpoint_read(1)
            if not got:
                break
            reads.append(got)
        assert self.o.ring_mem(1) == bytes(self.ring)
        self.pads = False
        self._snap(dict(kind="drain", reads=reads))
        return reads

    def disconnect(self):
        self.connected = False
        self._snap(dict(kind="disconnect"))

    def _flush(self):
        """rdma_flush retried while it makes progress (Pair.endpoint_write_continue): Send(slices + idx, byte_idx), the
        cursor walked over what was accepted, until done or a Send that takes nothing."""
        sl, _views, idx, bidx = self.wcur
        counts, done = [], False
        while not done:
            sent, w = self._one_send(sl[idx:], bidx)
            counts.append(sent)
            left = sent
            while left > 0:
                room = len(sl[idx]) - bidx
                if left >= room:
                    left -= room
                    idx += 1
                    bidx = 0
                else:
                    bidx += left
                    left = 0
            # (the cursor of the device: slice_idx = start + whole records, byte_idx inside the short one)
            done = idx >= len(sl)
            if sent == 0:
                break
        self.wcur = None if done else [sl, _views, idx, bidx]
        return counts, done

    def write(self, lens):
        assert self.wcur is None
        sl, views = self._mk(lens)
        self.wcur = [sl, views, 0, 0]
        counts, done = self._flush()
        self._snap(dict(kind="write", views=views, counts=counts, done=done))
        return counts, done

    def write_more(self):
        assert self.wcur is not None
        counts, done = self._flush()
        self._snap(dict(kind="write_more", counts=counts, done=done))
        return counts, done

    # -- family J: an asynchronous endpoint's write, one submit = one burst of up to sixteen Sends
    def begin(self, lens):
        assert self.asynchronous and self.wcur is None
        sl, views = self._mk(lens)
        self.wcur = [sl, views, 0, 0]
        self._snap(dict(kind="begin", views=views))

    def submit(self):
        """grdma_endpoint_write_submit + _write_test: with more slices left than max_sge, B = min(16, ceil(n / max_sge))
        Sends of max_sge slices from the cursor against one reading of the head (nobody drains meanwhile); else one."""
        sl, views, idx, bidx = self.wcur
        n = len(sl) - idx
        B = min(BURST_MAX, -(-n // self.max_sge)) if n > self.max_sge else 1
        per_send, total = [], 0
        for k in range(B):
            tail0 = self.tail
            sent, w = self._one_send(sl[idx:], bidx)
            w["burst_k"], w["folded"] = k, bidx if k == 0 else 0
            per_send.append(w)
            total += sent
            left = sent
            while left > 0:
                room = len(sl[idx]) - bidx
                if left >= room:
                    left -= room
                    idx += 1
                    bidx = 0
                else:
                    bidx += left
                    left = 0
            w["dry"] = sent == 0 and self.tail == tail0
        done = idx >= len(sl)
        self.wcur = None if done else [sl, views, idx, bidx]
        b = dict(B=B, sends=per_send, sent=total, done=done, cursor=(idx, bidx), n=n, burst=n > self.max_sge)
        self.bursts.append(b)
        self._snap(dict(kind="submit", sent=total, done=done, b=b))
        return b

    def abort(self):
        self.wcur = None
        self._snap(dict(kind="abort"))

    # -- steering
    def pieces(self, dist, biggest=None):
        """encoded sizes adding up to dist (a multiple of 8, 0 or >= 24), each what one Send takes whole"""
        assert dist % 8 == 0 and (dist == 0 or dist >= 24), dist
        big = biggest or (self.ring // 2 - 8) & ~7
        out = []
        while dist:
            p = dist if dist <= big else (big if dist - big >= 24 else dist - 24)
            out.append(p)
            dist -= p
        return out

    def prefill(self, nbytes):
        """nbytes of records into the ring, one record a Send, nothing read"""
        for p in self.pieces(nbytes):
            w = self.send([p - 16])
            assert w["fs"] is None, ("a prefill record does not fit", p, self.free0)
        return self

    def steer_tail(self, target):
        """the sender's tail at `target`, the ring empty: one record a Send, each drained at once"""
        dist = (target - self.tail) % self.ring
        if 0 < dist < 24:
            dist += self.ring
        for p in self.pieces(dist, biggest=(self.ring // 4) & ~7):
            w = self.send([p - 16])
            assert w["fs"] is None
            self.drain()
        assert self.tail == target % self.ring
        return self

    def finish(self):
        if not self.final:
            self.final = True
            self.o.close()
            self.o = None
        return self


def lens_to(total_enc, n):
    """n payload lengths (>= 1, every pad width from 0 to 7 among them) whose encoded sizes add up to total_enc"""
    assert total_enc % 8 == 0 and total_enc >= 24 * n, (total_enc, n)
    if n == 0:
        assert total_enc == 0
        return []
    q, r = divmod((total_enc - 24 * n) // 8, n)
    return [24 + 8 * (q + (1 if i < r else 0)) - 16 - i % 8 for i in range(n)]


# ----------------------------------------------------------------------------------------------------------------------
# Replay on the device
# ----------------------------------------------------------------------------------------------------------------------
class _States:
    def __init__(self, st):
        self.st = st

    def state(self, side):
        return self.st[side]


def _window_of(lib, pair):
    tx, rx = (C.c_uint64 * 16)(), (C.c_uint64 * 16)()
    assert lib.grdma_pair_last_dbg(pair.h, tx, rx) == 0
    return int(tx[7])


def _drain_all(b):
    out = []
    for _ in range(64):
        got, _wb = b.endpoint_read(8192)
        if not got:
            return out
        out += got
    raise AssertionError("the drain does not come to an end")


WRITE_DEADLINE = 30.0   # seconds one burst may take before the test fails


def run_on_device(g, script, wire, tag=""):
    """The finished script on a connected pair a -> b: after every step what the oracle showed after the same step."""
    lib = g.load()
    flags = WIRES[wire]
    R = script.ring
    a, b = mk_link(g, R, script.max_sge, flags)
    buf = g.DeviceBuffer(data=bytes(script.image) + bytes(16))
    keep = None
    try:
        if script.latency:
            a.set_latency_mode(True)
            b.set_latency_mode(True)
        if script.asynchronous:
            g._lib.check(lib.grdma_endpoint_set_async(a.h, 0, 0))
        for n, step in enumerate(script.steps):
            kind = step["kind"]
            at = "%s step %d (%s) on %s" % (tag, n, kind, wire)
            sl = [(buf.ptr + off, ln) for off, ln in step.get("views", ())]
            if kind == "send":
                w = step["w"]
                got = a.Send(sl, step["byte_idx"], MEM_DEVICE)
                assert got == step["sent"], (at, "accepted", got, step["sent"], w["fs"], w["short_pay"])
                if step["wrs"] is not None:
                    assert a.last_wrs() == step["wrs"], (at, a.last_wrs(), step["wrs"])
                    if flags == WIRE_STAGED and not script.latency:
                        exp = zlib.decompress(step["staging"])
                        assert _mask_pads(a.staging_mem(len(exp))) == _mask_pads(exp), (at, "staging image")
                if not script.latency:
                    win = _window_of(lib, a)
                    assert win == w["window"], (at, "priced window", win, "restated", w["window"], "guess", w["guess"],
                                                "m", w["m"], "fs", w["fs"])
            elif kind == "refused":
                arr, _k, _h = a._slices(sl)
                rc = lib.grdma_pair_send(a.h, arr, len(sl), 0, MEM_DEVICE)
                assert rc == -ERR_CAPACITY, (at, rc)
            elif kind == "drain":
                got = _drain_all(b)
                assert [len(x) for x in got] == [len(x) for x in step["reads"]], at
                assert got == step["reads"], at
            elif kind == "disconnect":
                a.Disconnect()
            elif kind == "write":
                got = a.endpoint_write(sl, MEM_DEVICE)
                assert got == (step["counts"], step["done"]), (at, got, step["counts"], step["done"])
            elif kind == "write_more":
                got = a.endpoint_write_continue()
                assert got == (step["counts"], step["done"]), (at, got, step["counts"], step["done"])
            elif kind == "begin":
                arr, _k, _h = a._slices(sl)
                keep = arr
                g._lib.check(lib.grdma_endpoint_write_begin(a.h, arr, len(sl), MEM_DEVICE))
            elif kind == "submit":
                g._lib.check(lib.grdma_endpoint_write_submit(a.h))
                done, sent = C.c_int(0), C.c_int64(0)
                t0 = time.time()
                while True:
                    rc = g._lib.check(lib.grdma_endpoint_write_test(a.h, C.byref(done), C.byref(sent)))
                    if rc == 1:
                        break
                    assert time.time() - t0 < WRITE_DEADLINE, (at, "the burst did not complete")
                assert (int(sent.value), bool(done.value)) == (step["sent"], step["done"]), \
                    (at, "summed sent / done", int(sent.value), bool(done.value), step["sent"], step["done"],
                     [(x["burst_k"], x["sent"], x["fs"]) for x in step["b"]["sends"]])
            elif kind == "abort":
                g._lib.check(lib.grdma_endpoint_write_abort(a.h))
                keep = None
            else:
                raise AssertionError(kind)
            ring = zlib.decompress(step["ring"])
            mem = b.ring_mem()
            if step["pads"]:
                assert _ring_eq(mem, ring), (at, "ring image")
            else:
                assert mem == ring, (at, "ring image", [i for i in range(R) if mem[i] != ring[i]][:8])
            if kind == "drain":
                assert mem == bytes(R), (at, "the drained ring is not all zero")
            check_state(a, b, _States(step["st"]))
            assert a.GetWritableSize() == step["writable"], (at, "GetWritableSize")
        del keep
    finally:
        a.close()
        b.close()
        buf.free()


# ----------------------------------------------------------------------------------------------------------------------
# The cases
# ----------------------------------------------------------------------------------------------------------------------
CASES = []   # dict(id, fam, build, needs, wires, slices)
_BY_ID = {}
_SCRIPTS = {}


def case(fam, name, needs, wires=("staged", "direct")):
    def reg(fn):
        c = dict(id="%s-%s" % (fam, name), fam=fam, build=fn, needs=needs, wires=tuple(wires))
        assert c["id"] not in _BY_ID, c["id"]
        CASES.append(c)
        _BY_ID[c["id"]] = c
        return fn
    return reg


def script_of(c):
    s = _SCRIPTS.get(c["id"])
    if s is None:
        s = _SCRIPTS[c["id"]] = c["build"]().finish()
    return s


def some(label, fn):
    """some Send of the script satisfies fn"""
    return (label, lambda s: any(fn(w) for w in s.sends))


def last(label, fn):
    """the last Send of the script satisfies fn"""
    return (label, lambda s: bool(s.sends) and fn(s.sends[-1]))


def some_burst(label, fn):
    return (label, lambda s: any(fn(b) for b in s.bursts))


def check_witnesses(c):
    s = script_of(c)
    assert s.steps[-1]["kind"] == "drain" and s.wcur is None, (c["id"], "a case ends drained: the ring all zero")
    missing = [label for label, fn in c["needs"] if not fn(s)]
    assert not missing, (c["id"], "misses its edge", missing,
                         [(w["m"], w["fs"], w["bound"], w["short_pay"], w["window"], w["end_rec"], sorted(w["end_at"]))
                          for w in s.sends][-4:])
    return s


def by_id(cid):
    return _BY_ID[cid]


def run_case(g, c, wire):
    run_on_device(g, check_witnesses(c), wire, tag=c["id"])


def ring_for(nbytes):
    """the smallest ring whose staging budget, less the 512 bytes a credit-bound case leaves unread, holds nbytes"""
    R = 64
    while R // 2 - 512 < nbytes:
        R *= 2
    return R


# ---- A: list length --------------------------------------------------------------------------------------------------
for _m in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4094, 4095):
    for _n in (1, 9):
        @case("A", "m%d_x%d" % (_m, _n),
              [last("all %d records whole" % _m, lambda w, m=_m: w["m"] == m and w["fs"] is None and w["whole"] == m),
               last("the window is what the restatement says", lambda w, m=_m: w["window"] == m)])
        def _a_len(m=_m, n=_n):
            s = Script(max(ring_for(m * enc(n) + 64), 1024), 4095)
            s.send([n] * m)
            s.drain()
            return s

for _sge in (30, 200, 4095):
    for _d in (-1, 0, 1):
        if _sge + _d > MAX_RECORDS:
            continue
        @case("A", "sge%d_count%+d" % (_sge, _d),
              [last("min(count, max_sge) records priced", lambda w, k=min(_sge, _sge + _d): w["m"] == k and w["whole"] == k),
               last("partial exactly when slices are left over", lambda w, sge=_sge: (w["offered"] > sge) == (w["sent"] < 5 * w["offered"]))])
        def _a_sge(sge=_sge, d=_d):
            s = Script(ring_for((sge + 1) * 24 + 64), sge)
            s.send([5] * (sge + d))
            s.drain()
            return s


@case("A", "count4096_refused", [last("the Send behind the refusal is whole", lambda w: w["m"] == 3 and w["fs"] is None)])
def _a_refused():
    s = Script(K16, 4095)
    s.send([40, 9])
    s.refused(MAX_RECORDS + 1)
    s.send([8, 1, 100])
    s.drain()
    return s


# ---- B: where the first short record falls ---------------------------------------------------------------------------
B_ROOM = {"exact": 64, "over": 64, "pay8": 32, "pay0": 24, "rounded": 88}


def place_short(s, fs, m, variant, tail_len=8):
    """the slice lengths of a Send of m slices on script s (as the oracle stands) whose record fs meets the budget's end:
    records 0 .. fs - 1 whole, `room` bytes of budget left in front of record fs"""
    room = B_ROOM[variant]
    room0 = s.room0
    if fs == 0:
        room = room0     # (nothing in front to steer with: the record is sized against the whole budget)
    wr = W(room)
    l = {"exact": wr, "over": wr + 1, "pay8": 100, "pay0": 5, "rounded": wr + 13}[variant]
    if fs == 0 and variant in ("pay8", "pay0"):
        assert wr == (8 if variant == "pay8" else 0), (variant, room0)
    assert l >= 1
    return lens_to(room0 - room, fs) + [l] + [tail_len] * (m - fs - 1)


def _b_needs(fs, m, variant, bound):
    want_bound = lambda w: w["bound"] == bound   # noqa: E731
    if variant == "exact":
        # the record at fs fits to the byte; whatever follows finds nothing left
        return [last("record %d fits exactly" % fs, lambda w: w["whole"] == fs + 1 and w["recs"][fs] == W(min(w["R"] // 2, w["free0"]) - sum(enc(x) for x in w["recs"][:fs]))),
                last("the next one, if any, gets nothing", lambda w: (w["fs"] is None and fs == m - 1) or (w["fs"] == fs + 1 and w["short_pay"] == 0 and want_bound(w)))]
    need = [last("first short record %d of %d" % (fs, m), lambda w: w["fs"] == fs and w["m"] == m and not w["zero"]),
            last("bound by %s" % bound, want_bound)]
    if variant == "over":
        need.append(last("one byte over", lambda w: w["short_pay"] >= 8 and w["short_pay"] % 8 == 0))
    elif variant == "pay8":
        need.append(last("short_pay 8", lambda w: w["short_pay"] == 8))
    elif variant == "pay0":
        need.append(last("short_pay 0: the record is not sent", lambda w: w["short_pay"] == 0 and len(w["recs"]) == fs))
    else:
        need.append(last("rounded down from a length that is no multiple of 8", lambda w: w["short_pay"] >= 8))
    return need


B_GRID = [(1, 256, fs) for fs in (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 255)] + \
         [(2, m, fs) for m in (300, 512) for fs in (126, 127, 128, 129, 255, 256, 257, m - 1)] + \
         [(16, 4095, fs) for fs in (1023, 1024, 1025, 4094)]
B_SKIPPED = []   # (per, m, fs, variant, bound): not constructible, see profiles/send_sweep.md

for _per, _m, _fs in B_GRID:
    for _variant in ("exact", "over", "pay8", "pay0", "rounded"):
        for _bound in ("staging", "credit", "equal"):
            if _fs == 0 and _variant in ("pay8", "pay0") and _bound != "credit":
                # record 0 has the whole budget in front of it: min(ring / 2, free) is 32 or 24 only when the free
                # space says so, i.e. bound by the credit (ring / 2 == 32 is family G's ring of 64 bytes)
                B_SKIPPED.append((_per, _m, _fs, _variant, _bound))
                continue

            @case("B", "per%d_m%d_fs%d_%s_%s" % (_per, _m, _fs, _variant, _bound),
                  _b_needs(_fs, _m, _variant, _bound) +
                  [last("runs of %d records a thread" % _per, lambda w, per=_per: w["per"] == per or w["window"] < w["m"])])
            def _b(m=_m, fs=_fs, variant=_variant, bound=_bound):
                R = max(ring_for(24 * (fs + 1) + 128), 4096)
                s = Script(R, 4095)
                if bound == "credit":
                    if fs == 0 and variant in ("pay8", "pay0"):
                        s.prefill(R - B_ROOM[variant])      # the free space itself is the 32 / 24 bytes
                    else:
                        s.prefill(R // 2 + 512)             # free0 = ring / 2 - 512, the receiver has not read
                elif bound == "equal":
                    s.prefill(R // 2)                       # free0 == ring / 2
                w = s.send(place_short(s, fs, m, variant))
                if bound == "equal":
                    assert w["free0"] == R // 2
                s.drain()
                return s


# ---- C: zero-length slices -------------------------------------------------------------------------------------------
def _c_zero_at(k):
    return last("the Send ends at the empty slice %d" % k, lambda w: w["zero"] and w["fs"] == k and w["short_pay"] == 0 and w["whole"] == k)


for _name, _lens, _k in (("first", [0, 8, 9], 0), ("middle", [8, 9, 1, 0, 40, 8], 3), ("last", [8, 9, 1, 40, 0], 4),
                         ("at_100_of_300", [9] * 100 + [0] + [9] * 199, 100), ("at_256_of_300", [3] * 256 + [0] + [3] * 43, 256)):
    @case("C", "zero_%s" % _name, [_c_zero_at(_k)])
    def _c_zero(lens=_lens):
        s = Script(K16, 4095)
        s.send(lens)
        s.drain()
        return s


@case("C", "zero_in_front_of_the_short_record",
      [last("the empty slice ends the Send in front of the record that would come up short", lambda w: w["zero"] and w["fs"] == 40)])
def _c_front():
    s = Script(K16, 4095)
    lens = place_short(s, 41, 60, "over")
    lens[40:41] = [0]       # slice 40 is empty, slice 41 is the one the budget would cut
    s.send(lens)
    s.drain()
    return s


@case("C", "zero_behind_the_short_record",
      [last("the budget ends the Send; the empty slice behind is never reached", lambda w: not w["zero"] and w["fs"] == 40 and w["short_pay"] > 0)])
def _c_behind():
    s = Script(K16, 4095)
    lens = place_short(s, 40, 60, "over")
    lens[41] = 0
    s.send(lens)
    s.drain()
    return s


@case("C", "zero_first_slice_then_the_rest",
      [some("an empty first slice takes nothing", lambda w: w["zero"] and w["fs"] == 0 and w["sent"] == 0 and w["byte_idx"] == 0),
       last("the list behind it goes out whole", lambda w: w["fs"] is None and w["m"] == 3)])
def _c_first_then():
    # (byte_idx above 0 into an empty slice is outside the reference's domain: pair.cc subtracts it from the length)
    s = Script(4096, 30)
    s.send([8, 40])
    s.send([0, 8, 9, 100], 0)
    s.send([8, 9, 100])
    s.drain()
    return s


# ---- D: the pricing window -------------------------------------------------------------------------------------------
def _d_prior(L):
    s = Script(K16, 4095)
    if L == 0:
        s.prefill(K16 - 24)            # 24 bytes free: at the reserve
        w = s.send([8])
        assert w["sent"] == 0 and not w["recs"]
    else:
        w = s.send(lens_to(24 * L + 8 * (L // 2), L))
        assert len(w["recs"]) == L
    s.drain()
    assert s.last_records == L
    return s, L + L // 4 + 64


for _L in (0, 1, 4, 100):
    _g = _L + _L // 4 + 64
    for _d in (-1, 0, 1):
        @case("D", "after%d_fs_guess%+d" % (_L, _d),
              [last("previous Send took %d records: guess %d" % (_L, _g), lambda w, L=_L, gg=_g: w["prev"] == L and w["guess"] == gg and w["m"] > gg),
               last("fs at guess %+d" % _d, lambda w, gg=_g, d=_d: w["fs"] == gg + d),
               last("inside the window: one pass" if _d < 0 else "outside the window: priced again over the whole list",
                    lambda w, gg=_g, d=_d: (w["window"] == gg and not w["repriced"]) if d < 0 else (w["window"] == w["m"] and w["repriced"]))])
        def _d_fs(L=_L, d=_d):
            s, guess = _d_prior(L)
            s.send(place_short(s, guess + d, guess + 40, "over"))
            s.drain()
            return s

        @case("D", "after%d_m_guess%+d_whole" % (_L, _d),
              [last("m at guess %+d, all whole" % _d, lambda w, L=_L, gg=_g, d=_d: w["m"] == gg + d and w["fs"] is None and w["prev"] == L and w["guess"] == gg),
               last("one pass when m <= guess, two above", lambda w, d=_d: w["window"] == w["m"] and w["repriced"] == (d > 0))])
        def _d_m(L=_L, d=_d):
            s, guess = _d_prior(L)
            s.send(lens_to(24 * (guess + d) + 8 * 7, guess + d))
            s.drain()
            return s

    @case("D", "after%d_none_short" % _L,
          [last("m above guess, nothing short: priced again", lambda w, gg=_g: w["m"] == gg + 40 and w["fs"] is None and w["repriced"] and w["window"] == w["m"])])
    def _d_none(L=_L):
        s, guess = _d_prior(L)
        s.send(lens_to(24 * (guess + 40) + 8 * 9, guess + 40))
        s.drain()
        return s


# ---- E: the ring's end -----------------------------------------------------------------------------------------------
E_AT = ("between", "header", "word1", "tile", "lastword", "behind_payload", "behind_last")
E_REC = ("first", "middle", "last_whole", "rec256", "short")


def _e_build(where, at):
    """-> (ring, lens, k, d): a Send whose record k holds the ring's end d bytes into its span, the tail steered to it"""
    tile = at == "tile"
    # the payload of the record that meets the end: 45 (five bytes in its last word); 48 where the padded payload ends
    # at the ring's end (a payload of whole words ends there itself: the strict side of the wrap test)
    big = TILE + 1000 + 5 if tile else (48 if at == "behind_payload" else 45)
    R = K64 if tile else K16
    if where == "first":
        k, n = 0, 6
    elif where == "middle":
        k, n = 5, 12
    elif where == "last_whole":
        k, n = 9, 10
    elif where == "rec256":
        k, n = 258, 270
    else:
        k, n = 20, 30       # the short record itself
    lens = [8 + i % 5 for i in range(n)]
    lens[k] = big
    return R, lens, k


def _e_offset(at, p):
    e = enc(p)
    return {"between": 0, "header": 8, "word1": 16, "tile": 8 + TILE, "lastword": e - 16, "behind_payload": e - 8, "behind_last": e}[at]


for _where in E_REC:
    for _at in E_AT:
        if _at == "behind_last" and _where not in ("last_whole", "short"):
            continue    # (behind any other record the end is "between" the next two)
        if _at == "between" and _where == "first":
            continue    # (the tail at 0: no end inside the Send)
        if _at == "lastword" and _where == "short":
            continue    # (a short payload is a multiple of 8: its last word is full, no pad behind the end)

        @case("E", "%s_%s" % (_where, _at),
              [last("the end %s" % _at, lambda w, at=_at: at in w["end_at"]),
               last("in record: %s" % _where,
                    lambda w, where=_where: w["end_rec"] is not None and
                    {"first": w["end_rec"] == 0, "middle": 0 < w["end_rec"] < w["whole"] - 1,
                     "last_whole": w["end_rec"] == w["whole"] - 1 and w["fs"] is None,
                     "rec256": w["end_rec"] >= 256, "short": w["fs"] is not None and w["short_pay"] > 0 and w["end_rec"] == w["fs"]}[where])])
        def _e(where=_where, at=_at):
            R, lens, k = _e_build(where, at)
            s = Script(R, 4095)
            if where == "short":
                # the budget (ring / 2) cuts record k to a payload we choose: records in front sized to leave `room`
                want = TILE + 1000 if at == "tile" else 40
                room = want + RESERVED
                lens = lens_to(R // 2 - room, k) + [want + 300] + [8] * 9
                p = want
            else:
                p = lens[k]
            x = sum(enc(n) for n in lens[:k])
            d = _e_offset(at, p)
            s.steer_tail(R - x - d)
            s.send(lens)
            s.drain()
            return s


# ---- F: byte_idx and the cursor --------------------------------------------------------------------------------------
for _len0, _bi in ((100, 1), (100, 99), (9, 8)):
    @case("F", "byte_idx%d_of_%d" % (_bi, _len0),
          [last("the first record is the rest of slice 0", lambda w, n=_len0 - _bi: w["byte_idx"] > 0 and w["recs"][0] == n and w["fs"] is None)])
    def _f_bi(len0=_len0, bi=_bi):
        s = Script(4096, 30)
        s.send([len0, 8, 41], bi)
        s.drain()
        return s


@case("F", "first_record_is_the_short_one",
      [last("record 0 comes up short behind byte_idx: the cursor stays in slice 0",
            lambda w: w["fs"] == 0 and w["short_pay"] > 0 and w["byte_idx"] == 7 and w["whole"] == 0)])
def _f_short0():
    s = Script(4096, 30)
    s.send([5000, 8], 7)
    s.drain()
    return s


@case("F", "endpoint_write_600_mixed",
      [some("a step cut by the budget inside a slice", lambda w: w["fs"] is not None and w["short_pay"] > 0),
       some("a step that begins inside a slice", lambda w: w["byte_idx"] > 0),
       some("a step that takes nothing", lambda w: w["sent"] == 0 and w["m"] > 0),
       some("a step of more than 256 slices", lambda w: w["m"] > 256),
       ("the write is done in the end", lambda s: s.wcur is None and s.steps[-2]["done"])])
def _f_write():
    s = Script(K16, 4095)
    lens = [(1, 9, 40, 700, 8, 255, 256, 257, 3000, 24, 13, 5000)[i % 12] for i in range(600)]
    _counts, done = s.write(lens)
    for _ in range(400):
        s.drain()
        if done:
            break
        _counts, done = s.write_more()
    assert done
    return s


# ---- G: oversize slices on the smallest rings ------------------------------------------------------------------------
for _R in (64, 256):
    for _name, _x in (("2R-1", 2 * _R - 1), ("2R", 2 * _R), ("2R+1", 2 * _R + 1), ("8R", 8 * _R), ("3R_4", 3 * _R // 4)):
        for _pos in ("first", "later"):
            @case("G", "r%d_%s_%s" % (_R, _name, _pos),
                  [some("a slice of %d bytes on a ring of %d comes up short" % (_x, _R),
                        lambda w, pos=_pos, R=_R: w["fs"] == (0 if pos == "first" else (1 if R == 64 else 2)) and not w["zero"]
                        and w["offered"] >= 2),
                   ("the slice goes out in pieces until nothing is left", lambda s: s.wcur is None)])
            def _g_over(R=_R, x=_x, pos=_pos):
                s = Script(R, 30)
                # (a ring of 64 bytes stages one record of at most 8 bytes a Send: the slice behind ONE small one)
                lens = [x, 3] if pos == "first" else ([3, x, 2] if R == 64 else [1, 3, x, 2])
                _counts, done = s.write(lens)
                for _ in range(200):
                    s.drain()
                    if done:
                        break
                    _counts, done = s.write_more()
                assert done
                return s


# ---- H: not connected ------------------------------------------------------------------------------------------------
@case("H", "disconnected_send_of_300",
      [some("a Send that left partial_write set", lambda w: w["fs"] is not None and w["m"] > 0),
       last("300 slices offered, none priced", lambda w: w["m"] == 0 and w["offered"] == 300 and w["sent"] == 0 and w["window"] == 0)])
def _h():
    s = Script(4096, 4095)
    s.send([40, 5000])          # comes up short: partial_write = 1, the tail has moved
    s.disconnect()
    s.send([9] * 300)
    s.drain()
    return s


# ---- I: latency mode, the block-wide plan with the inline copy -----------------------------------------------------------
def _i_case(name, needs, build):
    case("I", name, needs)(build)


def _i65():
    s = Script(K16, 4095, latency=True)
    s.send([8 + i % 7 for i in range(65)])
    s.drain()
    return s


def _i300():
    s = Script(K16, 4095, latency=True)
    s.send([1 + i % 13 for i in range(300)])
    s.drain()
    return s


def _i64k(extra):
    def build():
        s = Script(K256, 4095, latency=True)
        s.send([1024] * 63 + [1024 + extra])
        s.drain()
        return s
    return build


def _i_end():
    s = Script(K16, 4095, latency=True)
    lens = [9 + i % 6 for i in range(80)]
    x = sum(enc(n) for n in lens[:70])
    s.steer_tail(K16 - x - 16)
    s.send(lens)
    s.drain()
    return s


def _i_short():
    s = Script(K16, 4095, latency=True)
    s.send(place_short(s, 70, 90, "over"))
    s.drain()
    return s


_i_case("slices65", [last("65 slices: above one wave", lambda w: w["m"] == 65 and w["fs"] is None)], _i65)
_i_case("slices300", [last("300 slices", lambda w: w["m"] == 300 and w["fs"] is None)], _i300)
_i_case("slices64_64k", [last("64 slices of 64 KiB in all: the one-wave side of the guard",
                              lambda w: w["m"] == 64 and w["sent"] == SMALL_WAVE_BYTES and w["fs"] is None)], _i64k(0))
_i_case("slices64_64k_plus1", [last("64 slices of 64 KiB + 1: the block-wide side of the guard",
                                    lambda w: w["m"] == 64 and w["sent"] == SMALL_WAVE_BYTES + 1 and w["fs"] is None)], _i64k(1))
_i_case("ring_end_in_record70_of_80", [last("the ring's end one word into record 70's payload",
                                            lambda w: w["m"] == 80 and w["end_rec"] == 70 and "word1" in w["end_at"])], _i_end)
_i_case("short_record70_of_90", [last("record 70 of 90 comes up short", lambda w: w["fs"] == 70 and w["short_pay"] > 0)], _i_short)


# ---- J: the burst wave (k_tx_plan_seq) ------------------------------------------------------------------------------------
def _j_lens(n):
    return [(1, 8, 9, 3, 24, 5, 16, 7)[i % 8] for i in range(n)]


def _j_run(s, limit=40):
    """submits until the write is done, draining between bursts"""
    for _ in range(limit):
        b = s.submit()
        if b["done"]:
            return
        s.drain()
    raise AssertionError("the write does not come to an end")


for _sge in (30, 64, 65):
    for _name, _count in (("sge+1", _sge + 1), ("2sge", 2 * _sge), ("16sge", 16 * _sge), ("16sge+1", 16 * _sge + 1)) + \
            ((("above_1024", 1100),) if _sge == 64 else ()):
        _B = min(16, -(-_count // _sge))

        @case("J", "sge%d_%s" % (_sge, _name),
              [some_burst("a burst of %d Sends over %d slices" % (_B, _count), lambda b, B=_B, n=_count: b["B"] == B and b["n"] == n and b["burst"]),
               ("every slice goes out", lambda s: s.wcur is None and s.bursts[-1]["done"])] +
              ([some_burst("the seventeenth Send is left to the next submit", lambda b: b["B"] == 1 and not b["burst"] or b["n"] < 64)] if _name == "16sge+1" else []),
              wires=("direct",))
        def _j_count(sge=_sge, count=_count):
            s = Script(K64, sge, asynchronous=True)
            s.begin(_j_lens(count))
            _j_run(s)
            s.drain()
            return s


for _k, _kname, _slen in ((0, "first", 8), (2, "middle", 8), (3, "last", 8), (1, "second_inside_a_slice", 40)):
    @case("J", "short_in_send_%s" % _kname,
          [some_burst("Send %d of 4 is cut by the free space, every Send behind it is dry" % _k,
                      lambda b, k=_k: b["B"] == 4 and b["sends"][k]["fs"] is not None and b["sends"][k]["bound"] == "credit"
                      and all(x["fs"] is None for x in b["sends"][:k]) and all(x["dry"] for x in b["sends"][k + 1:])
                      and (k == 3 or b["sends"][k + 1]["dry"]))] +
          ([some_burst("the cut leaves the cursor inside a slice: the dry Sends report it",
                       lambda b, k=_k: b["B"] == 4 and b["sends"][k]["short_pay"] > 0 and b["sends"][3]["dry"] and b["cursor"][1] > 0)]
           if _slen > 8 else []),
          wires=("direct",))
    def _j_short(k=_k, slen=_slen):
        R, sge = 4096, 30
        s = Script(R, sge, asynchronous=True)
        # a first write fills the ring so that k Sends of 30 records and part of the next still fit: 15 records of 8 bytes
        # and a sixteenth that fits to the byte (nothing left for the next), or 10 of 40 bytes and 24 bytes of the next
        room = (k * sge + 15) * 24 + 32 if slen == 8 else (k * sge + 10) * enc(slen) + 48
        s.begin([p - 16 for p in s.pieces(R - room, biggest=1024)])
        _j_run_nodrain(s)
        s.begin([slen] * (4 * sge))
        s.submit()
        s.drain()
        _j_run(s)
        s.drain()
        return s


def _j_run_nodrain(s):
    for _ in range(40):
        b = s.submit()
        if b["done"]:
            return
        assert b["sent"] > 0, "the fill does not fit"
    raise AssertionError("the fill does not come to an end")


for _k in (0, 1):
    @case("J", "zero_length_in_send_%d" % _k,
          [some_burst("Send %d ends at an empty slice, the Sends behind it take nothing" % _k,
                      lambda b, k=_k: b["B"] == 3 and b["sends"][k]["zero"] and all(x["dry"] for x in b["sends"][k + 1:])
                      and b["sends"][k + 1]["zero"] and b["sends"][k + 1]["fs"] == 0)],
          wires=("direct",))
    def _j_zero(k=_k):
        s = Script(K16, 30, asynchronous=True)
        lens = _j_lens(90)
        lens[k * 30 + 11] = 0
        s.begin(lens)
        b = s.submit()
        assert not b["done"]
        s.abort()
        s.drain()
        return s


for _k, _at in ((0, "payload"), (0, "behind_payload"), (2, "payload"), (2, "behind_payload")):
    @case("J", "ring_end_in_send_%d_%s" % (_k, _at),
          [some_burst("the ring's end %s of a record of Send %d" % (_at, _k),
                      lambda b, k=_k, at=_at: b["burst"] and at in b["sends"][k]["end_at"] and b["sends"][k]["end_rec"] == 7)],
          wires=("direct",))
    def _j_end(k=_k, at=_at):
        s = Script(K16, 30, asynchronous=True)
        lens = _j_lens(100)
        p = 45 if at == "payload" else 48    # (48: the payload itself ends at the ring's end, the strict side of the wrap test)
        lens[k * 30 + 7] = p
        x = sum(enc(n) for n in lens[:k * 30 + 7])
        d = 24 if at == "payload" else enc(p) - 8
        # the tail is steered with writes of one record each, drained at once
        dist = (K16 - x - d) % K16
        for p in s.pieces(dist, biggest=2048):
            s.begin([p - 16])
            assert s.submit()["done"]
            s.drain()
        s.begin(lens)
        _j_run(s)
        s.drain()
        return s


@case("J", "byte_idx_folded_first_send_short_in_slice0",
      [some_burst("a burst that begins inside a slice and whose first Send stays inside it",
                  lambda b: b["burst"] and b["sends"][0]["folded"] > 0 and b["sends"][0]["fs"] == 0 and b["sends"][0]["short_pay"] > 0),
       ("every slice goes out", lambda s: s.wcur is None)],
      wires=("direct",))
def _j_fold():
    s = Script(4096, 30, asynchronous=True)
    s.begin([8, 9, 7000] + _j_lens(60))
    _j_run(s)
    s.drain()
    return s


FAMILIES = sorted({c["fam"] for c in CASES})


def cases(fam):
    return [c for c in CASES if c["fam"] == fam]


def tests():
    """-> [(case id, wire)]: one test each"""
    return [(c["id"], w) for c in CASES for w in c["wires"]]


def check_cases():
    for c in CASES:
        check_witnesses(c)
    return CASES


# ---- the emulated subset -------------------------------------------------------------------------------------------------
SUBSET_WIRE = {"E": "direct", "J": "direct"}   # (the split segment and the burst wave exist on the direct wire only)
# the cases a mutation of profiles/send_sweep.md was caught by alone
CAUGHT_ALONE = [("J-short_in_send_second_inside_a_slice", "direct")]   # the dry shortcut reporting byte_idx 0


def emu_subset():
    """The by-rule subset of the emulated run: of every family the smallest case (fewest slices in its script) that
    asserts more than parity -- the priced window of a blocking non-latency Send, families A to H; I and J are parity
    only, the smallest of each -- on the staged wire, E and J on the direct one, plus every case a mutation of
    profiles/send_sweep.md was caught by alone.  -> [(case id, wire)]"""
    out = []
    for fam in FAMILIES:
        small = min(cases(fam), key=lambda c: (script_of(c).nslices, c["id"]))
        out.append((small["id"], SUBSET_WIRE.get(fam, "staged")))
    for t in CAUGHT_ALONE:
        if t not in out:
            out.append(t)
    return out
