"""Shared by tests/test_zz_gpu_planner_sweep.py and tests/test_planner_sweep_emu.py: the case lists of the planner sweep,
the witnesses every case has to show from the oracle alone, and the driver that runs a case as a stream job.

A case is (family, payload pattern, repetitions, ring, max_sge, sends, promised); it runs on a schedule (sequential:
rxf_body / txf_body in k_rx_plan_job / k_tx_plan_job; paired: rxm_body / rxh_body / txm_body in k_plan_pair_mw) and a wire
(staged, direct).  The slice list is the pattern repeated, filled with non-zero position-dependent bytes.  Every list
is built from the constants the planner bodies branch on (RXF_MINRD 256, RXM_RESET 512, RXF_LOOKBACK 192, RXF_PMAX 512,
RXF_PER 4, RXM_CHUNK 256, the tile size), never sampled at random, except family I (fixed seed).

The reference is pyorc.OracleLink driven as tests/test_gpu_stream_job.py::_oracle_rounds drives it.  Rounds are kept at or
below ring / 6 bytes, where the paired schedule's Sends are never credit-limited and the oracle's plain rounds apply to both
schedules (as MULTI_CASES of that file).  Of the receiver's state the driver compares what a drain's commit writes:
head, moving_head, remain, internal_read_size, credit_msgs, leftover_cap (check_rx_state of that file) and total_read
against the payload bytes of the case times the passes.

WITNESSES.  In front of every drain the oracle gives the receiver's head, the sender's remote_tail, the read left open
(leftover_cap), internal_read_size, and -- from the send cursor -- the payload sizes of the round's records.  From these
alone `trace` derives per drain: V, the index F of the first record >= 512, the record whose span holds the ring end and
where in it the end falls, the record that takes the consumption past ring / 2, the read state in front of every record.
A case names the witnesses it needs; `check_witnesses` raises when one is missing, which the test modules call at
collection: a case cannot be silently vacuous."""
import ctypes as C
import random

from oracle import pyorc
from tests.stream_job_lib import PASSES, _advance, _fast_counts, _run_job, _table_cache_stats, check_rx_state, rx_state_of

MINRD, RESET, LOOKBACK, PMAX, PER, CHUNK = 256, 512, 192, 512, 4, 256
NONE = None   # (a witness that is absent: no such record in the drain)


def enc(n):
    return 16 + ((n + 7) & ~7)


def fill(n, k):
    """n non-zero bytes that depend on the position in the slice and on the slice's index."""
    base = _BASES.get(k)
    if base is None or len(base) < n:
        base = _BASES[k] = bytes(1 + (i * 7 + (i >> 4) * 13 + k * 29) % 255 for i in range(max(n, 16400)))
    return base[:n]


_BASES = {}
_FILLS = {}


def slices_of(pattern, reps):
    out = []
    for r in range(reps):
        for j, n in enumerate(pattern):
            key = (n, (r * len(pattern) + j) % 61)
            b = _FILLS.get(key)
            if b is None:
                b = _FILLS[key] = fill(n, key[1])
            out.append(b)
    return out


def space_after(n, s):
    """The endpoint-read state behind a record of n bytes (rdma_bp_posix.cc:180-291: reads of 256 bytes; a record that
    fills the open read and goes on takes a read of its own when 256 bytes or more are left, else opens a fresh one)."""
    if s == 0:
        return 0 if n >= MINRD else MINRD - n
    if n < s:
        return s - n
    if n == s:
        return 0
    r = n - s
    return 0 if r >= MINRD else MINRD - r


def branch(n, s):
    if s == 0:
        return "s0_n<256" if n < MINRD else ("s0_n==256" if n == MINRD else "s0_n>256")
    if n < s:
        return "n<s"
    if n == s:
        return "n==s"
    r = n - s
    return "n>s_r==255" if r == 255 else ("n>s_r==256" if r == 256 else ("n>s_r<255" if r < 255 else "n>s_r>256"))


def completes_slice(n, s):
    if s == 0:
        return n >= MINRD
    return n >= s


def _witness(R, head, tail, leftover, irs, sizes, per_send):
    Lr = (tail - head) % R
    es = [enc(n) for n in sizes]
    assert sum(es) == Lr, "the records of the send cursor are not what lies between head and remote_tail"
    w = {"V": len(sizes), "sizes": sizes, "head": head, "Lr": Lr, "leftover_in": leftover, "per_send": per_send}
    w["F"] = next((i for i, n in enumerate(sizes) if n >= RESET), NONE)
    # the ring end
    u = R - head
    w["wrap_rec"], w["wrap_at"] = NONE, "no_end"
    if u <= Lr:
        x = 0
        for i, e in enumerate(es):
            if u == x:
                w["wrap_at"], w["end_before"] = "between", i
                break
            if u < x + e:
                w["wrap_rec"] = i
                w["wrap_at"] = "header" if u - x == 8 else ("footer" if u - x == e - 8 else "payload")
                break
            x += e
        else:
            w["wrap_at"], w["end_before"] = "between", len(es)
    # the credit threshold: the first record whose end takes internal_read_size to ring / 2
    w["credit_rec"] = NONE
    thr, x = R // 2 - irs, 0
    for i, e in enumerate(es):
        x += e
        if x >= thr:
            w["credit_rec"] = i
            break
    # the read state in front of every record
    s = leftover
    w["branches"], w["states"] = set(), []
    first_done = NONE
    for i, n in enumerate(sizes):
        w["states"].append(s)
        w["branches"].add(branch(n, s))
        if first_done is NONE and completes_slice(n, s):
            first_done = i
        s = space_after(n, s)
    w["first_done"] = first_done
    w["leftover_out"] = s if s else MINRD
    return w


_TRACES = {}


def trace(case):
    """_oracle_rounds of tests/test_gpu_stream_job.py with the witnesses of every drain taken on the way.
    -> {"slices", "rounds", "st", "ring", "drains": [witness of every drain of the PASSES passes]}"""
    key = case.key()
    if key in _TRACES:
        return _TRACES[key]
    R, max_sge, sends = case.ring, case.max_sge, case.sends
    slices = case.slices()
    o = pyorc.OracleLink(R, max_sge)
    first_rounds, drains = None, []
    for _ in range(PASSES):
        idx, byte = 0, 0
        delivered, rounds = [], 0
        while idx < len(slices):
            sizes, per_send = [], []
            for _k in range(sends):
                if idx >= len(slices):
                    break
                q = o.p[0]
                free = R - ((q.remote_tail - q.status_recv.remote_head) % R)
                offered = min(len(slices) - idx, max_sge)
                sent = o.send(0, slices[idx:idx + max_sge], byte)   # (a Send takes at most max_sge slices of its list)
                left, n_rec, short = sent, 0, NONE
                start_byte = byte
                while left > 0:
                    room = len(slices[idx]) - byte
                    take = min(left, room)
                    sizes.append(take)
                    n_rec += 1
                    left -= take
                    if take == room:
                        idx += 1
                        byte = 0
                    else:
                        byte += take
                        short = take
                per_send.append({"records": n_rec, "byte_idx": start_byte, "short": short, "offered": offered,
                                 "whole": n_rec - (short is not NONE), "free_binds": free < q.staging_cap})
            rounds += 1
            w = _witness(R, o.p[1].ring.head, o.p[0].remote_tail, o.p[1].leftover_cap, o.p[1].internal_read_size, sizes, per_send)
            assert w["Lr"] <= R // 6 or not case.ring6, "a round of %d bytes on a ring of %d: above ring / 6" % (w["Lr"], R)
            while True:
                s, _alloc = o.endpoint_read(1)
                if not s:
                    break
                delivered.append(s)
            assert o.p[1].leftover_cap == w["leftover_out"], "the witness's read-state replay left the oracle's"
            drains.append(w)
            assert rounds < 100000
        if first_rounds is None:
            first_rounds = rounds
    out = {"slices": delivered, "rounds": first_rounds, "st": (o.state(0), rx_state_of(o)), "ring": o.ring_mem(1), "drains": drains}
    o.close()
    _TRACES[key] = out
    return out


# ---- witnesses: name -> predicate over the list of drains ---------------------------------------------------------
def some(pred):
    return lambda ds: any(pred(d) for d in ds)


def branches(*names):
    return lambda ds: set(names) <= set().union(*(d["branches"] for d in ds))


WITNESS = {
    "odd_open": some(lambda d: d["leftover_in"] not in (0, MINRD)),
    "no_slice_completes": some(lambda d: d["first_done"] is NONE),
    "read_state_branches": branches("n<s", "n==s", "n>s_r==255", "n>s_r==256", "s0_n<256", "s0_n==256", "s0_n>256"),
    "F==0": some(lambda d: d["F"] == 0),
    "F==1": some(lambda d: d["F"] == 1),
    "F==191": some(lambda d: d["F"] == 191),
    "F==192": some(lambda d: d["F"] == 192),
    "F==193_V>193": some(lambda d: d["F"] == 193 and d["V"] > 193),
    "noF_V==193": some(lambda d: d["F"] is NONE and d["V"] == 193),
    "noF_V==194": some(lambda d: d["F"] is NONE and d["V"] == 194),
    "run_above_lookback": some(lambda d: _longest_small_run(d["sizes"]) > LOOKBACK),
    "wrap_first": some(lambda d: d["wrap_rec"] == 0),
    "wrap_last": some(lambda d: d["wrap_rec"] is not NONE and d["wrap_rec"] == d["V"] - 1),
    "wrap_in_prefix": some(lambda d: d["wrap_rec"] is not NONE and d["F"] is not NONE and d["wrap_rec"] < d["F"]),
    "wrap_at_F": some(lambda d: d["wrap_rec"] is not NONE and d["wrap_rec"] == d["F"]),
    "wrap_behind_F": some(lambda d: d["wrap_rec"] is not NONE and d["F"] is not NONE and d["wrap_rec"] > d["F"]),
    "wrap_255": some(lambda d: d["wrap_rec"] == 255),
    "wrap_256": some(lambda d: d["wrap_rec"] == 256),
    "end_on_header": some(lambda d: d["wrap_at"] == "header"),
    "end_in_payload": some(lambda d: d["wrap_at"] == "payload"),
    "end_on_footer": some(lambda d: d["wrap_at"] == "footer"),
    "end_between": some(lambda d: d["wrap_at"] == "between"),
    "credit_first": some(lambda d: d["credit_rec"] == 0),
    "credit_last": some(lambda d: d["credit_rec"] is not NONE and d["credit_rec"] == d["V"] - 1),
    "credit_255": some(lambda d: d["credit_rec"] == 255),
    "credit_256": some(lambda d: d["credit_rec"] == 256),
    "credit_inside": some(lambda d: d["credit_rec"] is not NONE and 0 < d["credit_rec"] < d["V"] - 1),
    "tile_edges_in_a_big_drain": some(lambda d: d["V"] >= 128 and {8191, 8192, 8193, 16383, 16384, 16385} <= set(d["sizes"])),
    "four_sends": some(lambda d: len(d["per_send"]) == 4),
    "run193_at_i0": some(lambda d: _run193_at_i0(d["sizes"])),
    "send_begins_inside_a_slice": some(lambda d: any(p["byte_idx"] != 0 for p in d["per_send"])),
    "free_space_binds": some(lambda d: any(p["free_binds"] and p["records"] < p["offered"] + (p["short"] is not NONE) for p in d["per_send"])),
    "cut_leaves_nothing": some(lambda d: any(p["short"] is NONE and 0 < p["records"] < p["offered"] for p in d["per_send"])),
    "two_sends": some(lambda d: len(d["per_send"]) == 2),
}
for _v in (7, 30, 150, 405, 1000, 1001, 255, 256, 257, 258, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8190):
    WITNESS["V==%d" % _v] = some(lambda d, v=_v: d["V"] == v)
for _m in range(4):
    WITNESS["V%%4==%d" % _m] = some(lambda d, m=_m: d["V"] % PER == m and d["V"] > PER)
for _n in (8, 16):
    WITNESS["short_record_%d" % _n] = some(lambda d, n=_n: any(p["short"] == n for p in d["per_send"]))
for _r in (15, 16, 17):
    WITNESS["whole_records==%d" % _r] = some(lambda d, r=_r: any(p["whole"] == r and p["records"] <= p["offered"] and
                                                                 (p["short"] is not NONE or p["records"] < p["offered"])
                                                                 for p in d["per_send"]))


def _run193_at_i0(sizes):
    """a record >= 512, exactly 193 small ones behind it, and the next record (>= 512 or not) at an index that is a multiple
    of RXF_PER: the thread that owns it looks back over all 193"""
    for i, n in enumerate(sizes):
        if n >= RESET and i + 194 < len(sizes) and all(m < RESET for m in sizes[i + 1:i + 194]) and sizes[i + 194] >= RESET \
                and (i + 194) % PER == 0:
            return True
    return False


def _longest_small_run(sizes):
    best = run = 0
    for n in sizes:
        run = run + 1 if n < RESET else 0
        best = max(best, run)
    return best


class Case:
    """expect: {"sequential": e, "paired": e} with e one of "taken", ("declined", slot), ("never_taken",), "parity"."""

    def __init__(self, family, name, pattern, reps, ring, max_sge, need, expect, sends=1, promised=False, ring6=True, tables=False, lagged_on_direct=False, lagged_whole=None):
        self.family, self.name, self.pattern, self.reps, self.ring, self.max_sge = family, name, list(pattern), reps, ring, max_sge
        self.sends, self.promised, self.need, self.ring6 = sends, promised, list(need), ring6
        self.tables, self.lagged_on_direct, self.lagged_whole = tables, lagged_on_direct, lagged_whole
        self.expect = expect if isinstance(expect, dict) else {"sequential": expect, "paired": expect}

    def key(self):
        return (tuple(self.pattern), self.reps, self.ring, self.max_sge, self.sends)

    def slices(self):
        return slices_of(self.pattern, self.reps)

    def __repr__(self):
        p = self.pattern if len(self.pattern) <= 14 else self.pattern[:6] + ["..."] + self.pattern[-3:]
        return "%s/%s(pattern %s (P %d) x %d, ring %d, max_sge %d, sends %d, promised %s)" % (
            self.family, self.name, p, len(self.pattern), self.reps, self.ring, self.max_sge, self.sends, self.promised)


def check_witnesses(case):
    if case.lagged_on_direct:
        check_lagged_witnesses(case)
    ds = trace(case)["drains"]
    missing = [w for w in case.need if not WITNESS[w](ds)]
    assert not missing, "%r does not show %s (drains: V %s, F %s, wrap %s, credit %s)" % (
        case, missing, sorted({d["V"] for d in ds}), sorted({str(d["F"]) for d in ds}),
        sorted({"%s@%s" % (d["wrap_rec"], d["wrap_at"]) for d in ds}), sorted({str(d["credit_rec"]) for d in ds}))


# ---- the families -------------------------------------------------------------------------------------------------
K256, M1 = 1 << 18, 1 << 20
EDGES = [1, 8, 9, 247, 255, 256, 257, 511, 512, 513]
# Drains of a few records.  On the paired schedule every drain is laid out by a predicting body (rxm_body with a period,
# rxh_body from the Send's size table without one): taken.  On the sequential schedule rxf_body needs the period, which the
# general planner's search finds only in its bulk tier -- reached by a drain that still has records left once the wave
# tier has brought the read state to "between reads", with 512 free entries in the slice table; drains this small end
# inside the wave tier, so whether and when a period is known is not derivable: parity only.
TINY = {"sequential": "parity", "paired": "taken"}


def family_a():
    """Read-state machine (rxf_space_after / rxf_replay / rxf_lay).  The edge payloads in orders that make every branch
    occur; an odd max_sge leaves reads of capacity != 256 open in front of drains.  The documented contract (the state
    machine runs "from ANY starting state") says taken."""
    # 247 + 9 == 256 (n == s), 1 then 511 (n - s == 256), 1 then 510 ... the orders below are checked by their witnesses
    o1 = [247, 9, 1, 511, 512, 256, 8, 503, 255, 257, 513, 1, 510, 600]
    o2 = [513, 1, 8, 9, 247, 255, 256, 257, 511, 512]
    return [
        Case("A", "edges_every_branch", o1, 40, K256, 5, ["read_state_branches", "odd_open"], TINY),
        Case("A", "edges_every_branch_V255", o1, 150, M1, 255, ["read_state_branches", "odd_open", "V==255"], "taken"),
        Case("A", "edges_ascending_V257", o2, 200, M1, 257, ["odd_open", "V==257"], "taken"),
        Case("A", "edges_ascending_rotated", o2, 40, K256, 7, ["odd_open", "V==7"], TINY),
        # drains of three tiny records into an open read of 256: no slice completes in the drain (first_done == none);
        # every drain ends in a would-block with a short slice.  Drains of three records: see TINY (on the sequential
        # schedule rxf_body's first_done == none branch is reached by the V255 cases' drains only when one begins so).
        Case("A", "no_slice_completes", [1, 8, 9, 5], 12, K256, 3, ["no_slice_completes", "odd_open"], TINY),
    ]


def family_b():
    """Prefix region and look-back.  F (the first record >= 512) at drain index 0, 1, 191, 192 lies inside the prefix region:
    taken.  F at 193 with records behind it, in a stream whose runs of small records are longer than the look-back (200),
    and no such record at all among 194: declined, reason 4 -- on the sequential schedule this is the phase of rxf_body that
    shared its LDS flag with the probe.  No record >= 512 among 193: all of the drain is prefix region, taken."""
    out = []
    for f in (0, 1, 191, 192):
        # (a run of exactly f small records behind every 600, whole periods a drain and one record more: the second drain of
        # a pass begins right behind a 600 and meets the next one f records later)
        pat = [600] + [40] * f
        P = len(pat)
        out.append(Case("B", "F%d" % f, pat, max(13, 1500 // P), M1, max(2, 128 // P) * P + 1, ["F==%d" % f], "taken"))
    # period 201 with a run of 200; max_sge 2 * 201 + 8: the second drain of a pass begins 8 records into the period
    # (rxf_body's threads look back from i0 = 4 k: what declines these drains there is the run of 200 behind every 600, not
    #  F == 193 itself; rxm_body declines on F == 193 as such.  The look-back's exact length is pinned from both sides by
    #  run193_taken below and reset512_splits_run / F192.)
    out.append(Case("B", "F193", [600] + [40] * 200, 10, K256, 410, ["F==193_V>193", "run_above_lookback"], ("declined", 4)))
    # a run of exactly 193 small records whose successor sits at a multiple of RXF_PER in the drain: the longest run
    # rxf_body's look-back (192 steps back from the record in front of i0) still spans.  Sequential: taken.  Paired:
    # rxm_body's tables count 193 steps > RXF_LOOKBACK and decline by reason 4 whenever the drain goes on behind F.
    pat = [600] + [40] * 193
    out.append(Case("B", "run193", pat, 13, M1, 2 * len(pat) + 2, ["run193_at_i0"], {"sequential": "taken", "paired": ("declined", 4)}))
    # the first red case of the sweep as it was reported: V = 1001 over periods of 201
    out.append(Case("B", "run200_sge1001", [600] + [100] * 200, 30, M1, 1001, ["run_above_lookback", "V==1001"], ("declined", 4)))
    # a record of exactly RXM_RESET (2 * RXF_MINRD) bytes closes every read: it splits a run of 200 small records into two
    # of 100, inside the look-back.  (Compared with > instead of >= the run would be 201 and the bodies would decline.)
    pat = [600] + [40] * 100 + [512] + [40] * 100
    out.append(Case("B", "reset512_splits_run", pat, 13, M1, 2 * len(pat) + 1, ["V==405"], "taken"))
    out.append(Case("B", "small_only_V193", [40, 100, 24], 193 * 2, K256, 193, ["noF_V==193"], "taken"))
    # (sequential: a stream without a record that closes a read never reaches the general planner's bulk tier, no period is
    #  ever known and rxf_body has nothing to decline on: parity only)
    out.append(Case("B", "small_only_V194", [40, 100], 194 * 3, K256, 194, ["noF_V==194"],
                    {"sequential": "parity", "paired": ("declined", 4)}))
    return out


def family_c():
    """Period: P = 1, 2, 3, 511, 512 are within RXF_PMAX: taken.  P = 513 (all sizes distinct: no shorter period either) is
    above it: the periodic bodies never take it -- on the paired schedule the drains then go to rxh_body, which counts in the
    same slot: parity only there.  A detected period that is a multiple of the true one is what P1, P2 and P3 run with:
    the general planner's search keeps the LARGEST period up to 512 that the history supports (grdma_rx_plan.hip, "full
    search"), so a stream that repeats after 1, 2 or 3 records is laid out with a multiple of that."""
    out = []
    for name, pat in (("P1", [700]), ("P2", [600, 40]), ("P3", [600, 40, 300])):
        out.append(Case("C", name, pat, 1500 // len(pat), 2 * M1, 255, ["V==255"], "taken"))
    for P in (511, 512):
        out.append(Case("C", "P%d" % P, [520 + 8 * i for i in range(P)], 6, 8 * M1, 150, ["V==150"], "taken"))
    out.append(Case("C", "P513", [520 + 8 * i for i in range(513)], 6, 8 * M1, 150, ["V==150"], {"sequential": ("never_taken",), "paired": "parity"}))
    return out


def family_d():
    """Drain size through max_sge: around the RXF_PER thread boundary (V = 4 k + 0 .. 3), the RXM_CHUNK workgroup boundary
    (255 / 256 / 257, 511 / 512 / 513) and 4095: taken.  Rounds of two Sends with 4096, 4097 and 8190 records: parity only --
    whether rxm_body, rxh_body or the general planner lays out a round above RXM_G * RXM_CHUNK records depends on the planner
    pair's grid and on the period search's back-off, which the contract does not fix per drain."""
    out = []
    for v in (8, 9, 10, 11):
        out.append(Case("D", "V%d" % v, [600, 40, 300], 5 * v, K256, v, ["V%%4==%d" % (v % 4)], TINY))
    for v in (255, 256, 257, 258, 511, 512, 513):
        out.append(Case("D", "V%d" % v, [600, 40], v * 2, M1 if v < 300 else 2 * M1, v, ["V==%d" % v, "V%%4==%d" % (v % 4)], "taken"))
    out.append(Case("D", "V4095", [600, 40], 6192, 16 * M1, 4095, ["V==4095"], "taken"))
    return out


def family_d2():
    """Rounds of two Sends with 4096, 4097 and 8190 records of a periodic stream.  A job of two Sends a round launches
    RXM_G workgroups PER SEND (grdma_host_job.inc, job_groups: 32 x RXM_CHUNK = 8192 records), so these rounds are not above
    the drain's grid and rxm_body does not decline them by reason 2 -- with one Send a round max_sge cannot exceed 4095 and
    the reason-2 exit for "too many records" is not reachable from a job at all.  Paired: taken (as the 8190-record rounds of
    SENDS_CASES in tests/test_gpu_stream_job.py).  Sequential: the same small workgroups lay the round out (job_mw_seq), the
    contract states no taken rule for it: parity only.  rxh_body's second half is family I's."""
    e = {"sequential": "parity", "paired": "taken"}
    return [
        Case("D2", "V4096x2", [600, 40], 4096 + 50, 16 * M1, 2048, ["V==4096", "two_sends"], e, sends=2),
        Case("D2", "V4097x2", [600, 40, 300, 24, 80], (4098 + 4097) // 5, 16 * M1, 2049, ["V==4097", "two_sends"], e, sends=2),
        Case("D2", "V8190x2", [600, 40], 8190 + 60, 32 * M1, 4095, ["V==8190", "two_sends"], e, sends=2),
    ]


def family_e():
    """Ring end: the record that crosses it as a drain's first, its last, inside the prefix region, equal to F, behind F, and
    record 255 / 256 of a drain (a workgroup boundary of rxm_body); the end on the header word, in the payload, on the footer
    word and exactly between two records.  With the direct wire the same records are txm_body's / txf_body's wrap_rec.  The
    parameters were found by arithmetic over the encoded sizes; the witnesses check them from the oracle.  Taken."""
    return [
        Case("E", "walk_p3", [24, 8, 1000], 315, K256, 14, ["wrap_first", "wrap_at_F", "wrap_behind_F", "end_in_payload"], "taken"),
        Case("E", "walk_p4", [40, 100, 600, 1000], 188, K256, 12, ["wrap_last"], "taken"),
        Case("E", "walk_prefix", [600, 40, 300], 343, K256, 16, ["wrap_in_prefix"], "taken"),
        # encoded sizes 1032 + 1008: the first three ring ends fall between two records, on a header word, on a footer word
        Case("E", "walk_words", [1016, 992], 135, K256, 6, ["end_on_header", "end_on_footer", "end_between"], "taken"),
    ] + _wrap_chunk_cases()


def _wrap_chunk_cases():
    """V = 300 records of 336 bytes a pair; a lead of k pairs in front shifts which record of a drain meets the ring end."""
    out = []
    for want in (255, 256):
        pat, reps = WRAP_CHUNK[want]
        out.append(Case("E", "wrap_rec%d" % want, pat, reps, M1, 300, ["wrap_%d" % want], "taken"))
    return out


# (pattern and repetitions with which, at max_sge 300 on a 1 MiB ring, the ring end meets record 255 / 256 of a drain -- the
#  large record of the pair: found by a search over the oracle's trace, held by the witnesses)
WRAP_CHUNK = {255: ([40, 600], 833), 256: ([600, 40], 566)}


def family_f():
    """Credit threshold: the record that takes the consumption past ring / 2 as a drain's first, as its last, in between and
    as record 255 / 256, with the promised credit on and off (paired schedule; the sequential one has no such switch).
    Taken."""
    out = []
    for promised in (False, True):
        tag = "_promised" if promised else ""
        out.append(Case("F", "walk_p3" + tag, [24, 8, 1000], 315, K256, 14, ["credit_first", "credit_last", "credit_inside"], "taken",
                        promised=promised))
        for want in (255, 256):
            pat, reps = CREDIT_CHUNK[want]
            out.append(Case("F", "credit_rec%d%s" % (want, tag), pat, reps, M1, 300, ["credit_%d" % want], "taken", promised=promised))
    return out


CREDIT_CHUNK = {255: ([40, 600], 503), 256: ([600, 40], 502)}


def family_g():
    """Table cache and stale state (rxm_body's eight slots behind the record-size history; the period, the strikes and the
    back-off of the general planner's search).  rotations9: nine distinct sizes at max_sge 1000 (= 1 mod 9) -- every drain begins at another
    of nine rotations, more than the slots hold, so slots are evicted and filled again: taken.  stale: on ONE connection
    pattern A, then B with the same period and other sizes, then a pattern with another period, then A again, three passes:
    parity only (at every change the bodies decline until the search has the new period).  On the paired schedule
    grdma_rx_table_cache_stats must show hits and fills for both."""
    a, b, c = [600, 40, 300], [700, 24, 200], [600, 40]
    return [
        Case("G", "rotations9", [520, 600, 680, 760, 840, 920, 1000, 1080, 1160], 1400, 8 * M1, 1000, ["V==1000"], "taken", tables=True),
        Case("G", "stale", a * 1200 + b * 1200 + c * 1800 + a * 1200, 1, 4 * M1, 512, ["V==512"], "parity", tables=True),
    ]


def family_h():
    """Tiles: payloads around the 8 KiB tile (rings below 32 MiB) and the 16 KiB one (a 32 MiB ring).  edges_V129*: every
    tile-edge payload with a 40-byte record behind it, drains of 129 records -- large enough for the period to be known on
    both schedules, so rxf_body / rxf_lay / rxf_tiles lay these payloads out: taken.  tile8k / tile16k: drains of five
    records, see TINY."""
    pat = [8191, 8192, 8193, 16383, 16384, 16385]
    mixed = [x for n in pat for x in (n, 40)]
    return [
        Case("H", "tile8k", pat, 8, M1, 5, [], TINY),
        Case("H", "tile16k_ring32m", pat, 3, 32 * M1, 5, [], TINY),
        Case("H", "edges_V129", mixed, 44, 8 * M1, 129, ["tile_edges_in_a_big_drain"], "taken"),
        Case("H", "edges_V129_ring32m", mixed, 44, 32 * M1, 129, ["tile_edges_in_a_big_drain"], "taken"),
    ]


def _seeded(n, values):
    rng = random.Random(20260)
    return [rng.choice(values) for _ in range(n)]


def family_i():
    """No period (rxh_body on the paired schedule; the general planner on the sequential one): sizes drawn with a fixed seed
    from the edge values of A and H, one Send per round and two; rounds of exactly 4096 records (RXH_HALF: the first half of
    the size table), of 4097 and of 8190 (its second half), small edge values only, to keep the round inside ring / 6.
    Sequential: parity only (no period, nothing for rxf_body).  Paired, rounds of at most 4096 records: every drain of
    the graph passes is rxh_body's -- the rule of test_drains_without_a_period_are_predicted_from_the_sends_sizes: taken >=
    (PASSES - 1) * rounds - 2.  Above 4096 records rxh_body leaves a round to the general planner while its period search
    is due (five times at first, grdma_rx_hint.h: search_due): five less."""
    sizes = _seeded(180, EDGES + [600, 1000, 8191, 8192, 8193, 16383, 16384, 16385])
    return [
        Case("I", "edges_seeded", sizes, 1, 2 * M1, 30, ["V==30"], {"sequential": "parity", "paired": ("taken_min", 2, 0)}),
        Case("I", "edges_seeded_x2", sizes, 1, 2 * M1, 20, ["two_sends"], {"sequential": "parity", "paired": ("taken_min", 2, 0)}, sends=2),
        Case("I", "V4096x2", _seeded(4096 * 3, EDGES), 1, 16 * M1, 2048, ["V==4096", "two_sends"],
             {"sequential": "parity", "paired": ("taken_min", 2, 0)}, sends=2),
        Case("I", "V4097x2", _seeded(4098 * 3 + 4097, EDGES), 1, 16 * M1, 2049, ["V==4097", "two_sends"],
             {"sequential": "parity", "paired": ("taken_min", 2, 5)}, sends=2),
        Case("I", "V8190x2", _seeded(8190 * 3, EDGES), 1, 32 * M1, 4095, ["V==8190", "two_sends"],
             {"sequential": "parity", "paired": ("taken_min", 2, 5)}, sends=2),
    ]


def family_j():
    """Send pricing (txf_body on the sequential schedule, txm_body on the paired one).
    m2047 / m2048 / m2049: the slices a Send is offered around TXM_WIN (through max_sge).  Taken.
    cut_*: Sends cut by min(staging budget, free space) on a ring the rounds fill -- in the oracle's plain rounds the drain has
    emptied the ring before every Send, so the staging budget (ring / 2) is what binds; the cut is the same formula.  Whole
    records per Send 15 / 16 / 17 (around the 16 entries between two samples of the index), the short record with payload
    8 and 16, the cut that leaves nothing (43 records of 3048 bytes end 8 bytes below the budget), Sends that begin inside
    a slice.  These rounds are above ring / 6.  Paired / staged runs them with the promised credit, where the schedule
    equals the plain rounds.  The promised credit is a staged-wire mode (grdma_host_job.inc, job_promise: with a direct
    wire the gather of round t + 1 writes the ring in the launch of round t's scatter), so paired / direct sees its credit
    a round late and is run against the oracle driven that way (run_case_lagged: a sequential pass, then the paired
    chain) -- there the FREE SPACE is what cuts the Sends, which the lagged trace witnesses.  Parity only: the records are cut at other places every round, there is no period for the bodies to take.
    folded: four Sends per round priced as one cut of the index."""
    out = []
    for m in (2047, 2048, 2049):
        out.append(Case("J", "m%d" % m, [600, 40], m + m // 2 + 30, 4 * M1, m, ["V==%d" % m], "taken"))
    out += [
        Case("J", "cut_15_short8_16", [8720], 60, K256, 30, ["whole_records==15", "short_record_8", "short_record_16",
                                                              "send_begins_inside_a_slice"], "parity", promised=True, ring6=False, lagged_on_direct=True),
        Case("J", "cut_16_17", [7696], 60, K256, 30, ["whole_records==16", "whole_records==17", "send_begins_inside_a_slice"], "parity",
             promised=True, ring6=False, lagged_on_direct=True),
        Case("J", "cut_leaves_nothing", [3032], 180, K256, 60, ["cut_leaves_nothing"], "parity", promised=True, ring6=False, lagged_on_direct=True),
    ] + [
        # the free space (credit a round late) cuts a Send behind 15 / 16 / 17 whole records: paired / direct, lagged trace
        Case("J", "free_cut_%d" % k, [n], max(60, 200000 // n), K256, 30, [], "parity", promised=True,
             ring6=False, lagged_on_direct=True, lagged_whole=k) for k, n in ((15, 5216), (16, 3680), (17, 3632))
    ] + [
        Case("J", "folded_sends", [600, 40, 300], 40, M1, 7, ["four_sends"], "parity", sends=4),
    ]
    return out


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "D2": family_d2, "E": family_e, "F": family_f,
            "G": family_g, "H": family_h, "I": family_i, "J": family_j}
SCHEDULES = ["sequential", "paired"]
WIRES = ["staged", "direct"]


def cases(family):
    return FAMILIES[family]()


TARGET = {"A": "sequential", "B": "sequential", "C": "sequential", "D": "sequential", "E": "sequential", "H": "sequential",
          "J": "sequential", "D2": "paired", "F": "paired", "G": "paired", "I": "paired"}


def emu_subset():
    """The by-rule subset of the emulated run: of every family the smallest case (fewest slices) that asserts more than
    parity on the schedule whose bodies the family targets (TARGET: rxf_body / txf_body on the sequential schedule;
    rxm_body, rxh_body, the table cache and the promised credit on the paired one) -- of family F a promised-credit case,
    of J (parity only) the smallest -- plus family B's F = 193 case on the sequential schedule.
    -> [(family, case name, schedule, wire)]"""
    out = []
    for fam in sorted(FAMILIES):
        cs, sched = cases(fam), TARGET[fam]
        more = [c for c in cs if c.expect[sched] != "parity" and (fam != "F" or c.promised)]
        small = min(more or cs, key=lambda c: (len(c.pattern) * c.reps, c.name))
        out.append((fam, small.name, sched, "staged"))
    out.append(("B", "F193", "sequential", "staged"))
    return out


# ---- the driver ---------------------------------------------------------------------------------------------------
def lagged_trace(case):
    """The oracle driven as the paired chain without the promised credit runs a job (tests/test_gpu_stream_job.py,
    _oracle_sequential_then_paired): pass 1 sequential, pass 2 with Send k priced with the credits of the drains <= k - 2.
    -> first-pass slices and rounds, second-pass slices, rounds given, state, ring, and per Send of pass 2 whether the free
    space was below the staging budget and how many whole records went out."""
    key = ("lagged",) + case.key()
    if key in _TRACES:
        return _TRACES[key]
    R, slices = case.ring, case.slices()
    o = pyorc.OracleLink(R, case.max_sge)

    def drain(out):
        while True:
            s, _alloc = o.endpoint_read(1)
            if not s:
                return
            out.append(s)
    idx, byte, rounds, first = 0, 0, 0, []
    while idx < len(slices):
        idx, byte = _advance(slices, idx, byte, o.send(0, slices[idx:idx + case.max_sge], byte))
        rounds += 1
        drain(first)
        assert rounds < 100000
    paired_rounds = 2 * rounds + 6
    sender = o.p[0]
    latest = start = sender.status_recv.remote_head
    views, delivered, sends, idx, byte = [], [], [], 0, 0
    for k in range(paired_rounds):
        if idx >= len(slices):
            break
        lagged = start if k < 2 else views[k - 2]
        sender.status_recv.remote_head = lagged
        free = R - ((sender.remote_tail - lagged) % R)
        i0, offered = idx, min(len(slices) - idx, case.max_sge)
        idx, byte = _advance(slices, idx, byte, o.send(0, slices[idx:idx + case.max_sge], byte))
        sends.append({"free_binds": free < sender.staging_cap, "whole": idx - i0, "cut": byte != 0,
                      "short_of_offer": byte != 0 or idx - i0 < offered})
        drain(delivered)
        if sender.status_recv.remote_head != lagged:
            latest = sender.status_recv.remote_head
        views.append(latest)
    assert idx == len(slices), "the rounds given to the paired pass do not carry the whole list"
    sender.status_recv.remote_head = latest
    out = {"first": first, "rounds": rounds, "slices": delivered, "paired_rounds": paired_rounds, "used": len(sends),
           "st": (o.state(0), rx_state_of(o)), "ring": o.ring_mem(1), "sends": sends}
    o.close()
    _TRACES[key] = out
    return out


def check_lagged_witnesses(case):
    t = lagged_trace(case)
    assert any(p["free_binds"] and p["short_of_offer"] for p in t["sends"]), "%r: no Send of the paired pass is cut by the free space" % case
    if case.lagged_whole is not None:
        assert any(p["free_binds"] and p["short_of_offer"] and p["whole"] == case.lagged_whole for p in t["sends"]), \
            "%r: no Send cut by the free space behind %d whole records" % (case, case.lagged_whole)


def run_case_lagged(g, case, wire):
    """A cut case on the paired schedule WITHOUT the promised credit, against lagged_trace: the flow of
    test_paired_schedule_at_a_credit_limited_ring_equals_the_oracle_with_the_credit_one_round_late."""
    from grpc_rdma_amd import stream as gs
    import random as _r
    exp = lagged_trace(case)
    tag = "%r on paired (credit a round late) / %s" % (case, wire)
    R, slices = case.ring, case.slices()
    rng = _r.Random(5)
    bufs = [g.DeviceBuffer(data=s, offset=rng.randrange(16)) for s in slices]
    flags = 2 if wire == "direct" else 0
    tx, rx = g.Pair(R, case.max_sge, flags), g.Pair(R, case.max_sge, flags)
    g.connect_pairs(tx, rx)
    try:
        N = sum(len(s) for s in slices)
        dst_cap = N + 32 * (2 * len(slices) + 64) + 4096
        dst = g.DeviceBuffer(nbytes=dst_cap)
        sge = [(b.ptr, len(s)) for b, s in zip(bufs, slices)]
        job = gs.MultiStreamJob([(tx, rx, sge, dst.ptr, dst_cap, 2 * len(slices) + 64)], 4096)
        job.set_pipeline(False)
        r = job.run(gs.RUN_EAGER)
        assert r.done and r.bytes_delivered == N, tag
        assert int(max(r.tx_rounds, r.rx_rounds)) == exp["rounds"], tag
        mem = dst.read(dst_cap)
        assert [mem[o:o + n] for o, n in job.delivered_slices(0)] == exp["first"], tag
        job.set_pipeline(True)
        job.set_rounds(exp["paired_rounds"])
        r = job.run(gs.RUN_GRAPH)
        assert r.done and r.bytes_delivered == N and r.bytes_sent == N, tag
        mem = dst.read(dst_cap)
        got = [mem[o:o + n] for o, n in job.delivered_slices(0)]
        assert [len(x) for x in got] == [len(x) for x in exp["slices"]], tag
        assert got == exp["slices"], tag
        assert rx.ring_mem() == exp["ring"] == bytes(R), tag
        txs, rxs = tx.state(), rx.state()
        for k in ("remote_tail", "remote_head", "partial_write"):
            assert txs[k] == exp["st"][0][k], (k, tag)
        check_rx_state(rxs, exp["st"][1], tag, total_read=2 * N)   # (two passes: the sequential one, the paired chain)
        job.close()
    finally:
        tx.close()
        rx.close()


def run_pool_recycle(g, wire):
    """Family G across a PairPool recycle: pattern A on a pair taken from the pool, the pair put back, a pair taken again
    under other ids -- built from the same blocks -- and pattern B (A's period, other sizes), then A's again on a third
    take.  A recycled pair must carry nothing over: period, history, strikes / back-off and table slots are the
    connection's, and each job has to equal the oracle's rounds on a FRESH link, taken drains included."""
    lib = g.load()
    R, SGE, flags = 4 * M1, 512, 2 if wire == "direct" else 0
    a, b = [600, 40, 300], [700, 24, 200]
    lib.grdma_pair_pool_trim()
    assert lib.grdma_pair_pool_reserve(2, R, SGE, flags, 0) == 0
    try:
        for lap, pat in enumerate((a, b, a)):
            case = Case("G", "pool_lap%d" % lap, pat, 1200, R, SGE, ["V==512"], "taken", tables=True)
            check_witnesses(case)
            ids = (b"sweep-tx-%d" % lap, b"sweep-rx-%d" % lap)
            stats0 = (C.c_uint64 * 5)()
            lib.grdma_pair_pool_stats(stats0)
            ha, hb = lib.grdma_pair_pool_take(ids[0], R, SGE, flags), lib.grdma_pair_pool_take(ids[1], R, SGE, flags)
            assert ha and hb
            stats1 = (C.c_uint64 * 5)()
            lib.grdma_pair_pool_stats(stats1)
            assert stats1[2] > stats0[2], "lap %d: the pairs were not built from pooled blocks" % lap
            tx, rx = g.Pair(R, SGE, flags, handle=ha), g.Pair(R, SGE, flags, handle=hb)
            g.connect_pairs(tx, rx)
            try:
                assert rx.ring_mem() == bytes(R), "lap %d: a recycled ring was not zeroed" % lap
                run_case(g, case, "paired", wire, pairs=(tx, rx))
            finally:
                tx.detach()
                rx.detach()
                lib.grdma_pair_pool_putback(ha)
                lib.grdma_pair_pool_putback(hb)
    finally:
        lib.grdma_pair_pool_trim()


def run_case(g, case, schedule, wire, pairs=None):
    """Runs the case as a stream job (three passes on one connection) and asserts the oracle's slices, ring image and state
    and the family's taken / declined rule.  Assertion messages carry the case."""
    paired = schedule == "paired"
    if paired and wire == "direct" and case.lagged_on_direct:
        return run_case_lagged(g, case, wire)
    exp = trace(case)
    before, tab0 = _fast_counts(g), _table_cache_stats(g)
    read0 = pairs[1].state()["total_read"] if pairs is not None else 0
    got = _run_job(g, case.ring, case.max_sge, case.slices(), pipeline=paired, flags=2 if wire == "direct" else 0,
                   sends=case.sends, promise=case.promised and paired, pairs=pairs)
    after, tab1 = _fast_counts(g), _table_cache_stats(g)
    tag = "%r on %s / %s" % (case, schedule, wire)
    assert [len(x) for x in got["slices"]] == [len(x) for x in exp["slices"]], tag
    assert got["slices"] == exp["slices"], tag
    if not paired and case.sends == 1:   # (the job counts Sends: with several a round the count is an upper bound)
        assert got["rounds"] == exp["rounds"], tag
    assert got["ring"] == exp["ring"] == bytes(case.ring), tag
    st0, st1 = exp["st"]
    for k in ("remote_tail", "remote_head", "partial_write"):
        assert got["tx"][k] == st0[k], (k, tag)
    check_rx_state(got["rx"], st1, tag, total_read=read0 + PASSES * sum(case.pattern) * case.reps)
    delta = [a - b for a, b in zip(after, before)]
    e = case.expect[schedule]
    if e == "taken":
        assert delta[0] >= exp["rounds"], "drains taken %d of %d rounds a pass (declined by reason %s): %s" % (
            delta[0], exp["rounds"], delta[1:6], tag)
    elif e == ("never_taken",):
        assert delta[0] == 0, "drains taken %d (declined by reason %s): %s" % (delta[0], delta[1:6], tag)
    elif isinstance(e, tuple) and e[0] == "declined":
        others = [delta[k] for k in (2, 3, 4, 5) if k != e[1]]
        assert delta[e[1]] >= 1 and not any(others), "declined by reason %s, expected slot %d alone: %s" % (delta[1:6], e[1], tag)
    elif isinstance(e, tuple) and e[0] == "taken_min":
        want = max(1, e[1] * exp["rounds"] - 2 - e[2])
        assert delta[0] >= want, "drains taken %d, at least %d expected of %d rounds a pass (declined by reason %s): %s" % (
            delta[0], want, exp["rounds"], delta[1:6], tag)
    else:
        assert e == "parity", e
    if case.tables and paired:
        hits, fills = tab1[0] - tab0[0], tab1[1] - tab0[1]
        assert hits >= 1 and fills >= 1, "table cache hits %d, fills %d: %s" % (hits, fills, tag)
    return delta
