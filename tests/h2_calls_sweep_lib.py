"""The call table (k_h2_calls_*, csrc/grdma_h2_calls.h) swept over tables built from the constants its stages branch
on: the 64 lanes of a wave (the keyed ranks), the 256 descriptors a workgroup takes at a time (the waves' turns at the
count rows), a workgroup's run and the grid of 64 x 256 lanes (2 x 256 under the emulator), the table's mask and its half,
the 4097 keys of the counting sort.

A case is a deterministic script of steps on one CH harness (tests/h2_calls_lib.py): (reqs, msgs, events, now[, caps]).
The reference is tests/h2_calls_model.CallsModel; CH.step compares the dispatch table, the segment words and the done
list whole with their fill, the result block, the dump and the counters exactly.  Nothing here has a tolerance.

Every case names the edge it is there for, and a witness -- computed from the model alone (simulate) -- shows that the
case reaches it; check_cases() runs them all.  pytest rewrites no `assert` in a helper module: checks go through `same`."""
import copy

from tests.h2_calls_lib import BIG, cluster_id
from tests.h2_calls_model import (DEADLINE, EXPIRED_MSG, FIRST, LAST, LEFT, LOST, READS_CLOSED, CallsModel, closed, message, request)
from tests.h2_device_lib import same

WAVE, THREADS, GRID, EMU_GRID, KEYS = 64, 256, 64, 2, 4097  # H2C_THREADS, H2C_GRID, H2C_KEYS_MAX of csrc/grdma_h2_calls.h
EMU_MAX = 3000  # a case with at most this many rows in all its tables also runs under the emulator

CASES = []


def case(name, edge, steps, wit, slots=0, nmethods=1):
    CASES.append(dict(id=name, edge=edge, steps=steps, wit=wit, slots=slots, nmethods=nmethods))


def sid(k):
    return 2 * k + 1


def run_len(n, grid):
    """the length of a workgroup's run of n items (h2c_run)"""
    per = -(-n // grid)
    return -(-per // THREADS) * THREADS


def seqs(disp, stream):
    return [r[7] for r in disp if r[3] == stream and r[5] != 0xffffffff]


# ---- the keyed ranks of a wave: one stream at chosen lanes, every lane another stream, every lane the same ------------------
for lanes in ((0, 63), (31, 32), (0, 1, 2, 61, 62, 63)):
    case("wave_lanes_%s" % "_".join(map(str, lanes)), "a stream's messages at the lanes %r of one wave, 63 other streams between" % (lanes,),
         [([request(sid(k), k % 3) for k in range(64)], [message(1 if i in lanes else sid(1 + i), length=i) for i in range(64)], [closed(1, False)], 0)],
         lambda sim, lanes=lanes: seqs(sim[0][0], 1) == list(range(len(lanes))) and [r[4] for r in sim[0][0] if r[6] & LAST] == [lanes[-1]],
         slots=256, nmethods=3)
case("wave_every_lane_its_own_stream", "64 keys in one wave: the keyed loop's longest trip",
     [([request(sid(k), 0) for k in range(64)], [message(sid(63 - i)) for i in range(64)], [], 0)],
     lambda sim: all(r[6] & FIRST for r in sim[0][0]) and sim[0][3][1] == 64, slots=256)
case("wave_every_lane_one_stream", "one key in every lane of four waves: the waves' turns carry the count",
     [([request(1, 0)], [message(1, length=i) for i in range(THREADS)], [], 0)],
     lambda sim: seqs(sim[0][0], 1) == list(range(THREADS)))
# ---- the 256 of a workgroup, its run, the grid -----------------------------------------------------------------------------------
for n in (THREADS + 1, run_len(EMU_GRID * THREADS + 1, EMU_GRID) + 1, GRID * THREADS + 1):
    case("one_stream_over_%d_descriptors" % n, "a call's count across the waves of a trip, the trips of a run and the runs (%d descriptors)" % n,
         [([request(1, 1), request(3, 0)], [message(1 if i % 3 else 3, length=i % 7) for i in range(n)], [closed(3, True)], 0)],
         lambda sim, n=n: seqs(sim[0][0], 1) == list(range(n - (n + 2) // 3)) and sim[0][1] == [0, (n + 2) // 3, n, n], nmethods=2)
case("records_two_runs_duplicates_across", "a stream's two requests in different runs of the records: the lower record wins",
     [([request(sid(k % 600), k // 600) for k in range(1200)], [message(sid(k)) for k in (0, 599)], [], 0)],
     lambda sim: sim[0][3][0] == 600 and [r[5] for r in sim[0][0]] == [0, 0] and run_len(1200, EMU_GRID) < 1200 <= GRID * THREADS, slots=2048, nmethods=2)
case("events_across_runs", "the closes of a step in three runs of the events, in event order behind the deadlines",
     [([request(sid(k), 0, timeout=k % 2 * 50) for k in range(300)], [], [], 10),
      ([], [], [closed(sid(j % 300), j >= 300) for j in range(600)], 60)],
     lambda sim: [d[5] & 0xff for d in sim[1][2]] == [DEADLINE] * 150 + [READS_CLOSED] * 300 + [LEFT] * 300 and sim[1][3][5] == 0, slots=1024)
# ---- the table's mask and its half ---------------------------------------------------------------------------------------------------
case("mask_one_home_eight_deep", "eight ids on home 15 of 16 slots: every probe wraps; one more is lost; a LEFT makes room",
     [([request(cluster_id(15, k), 0) for k in range(9)], [message(cluster_id(15, k)) for k in range(9)], [closed(cluster_id(15, 0), True)], 0),
      ([request(cluster_id(15, 8), 0)], [message(cluster_id(15, k)) for k in range(9)], [], 0)],
     lambda sim: sim[0][3][:3] == (8, 8, 1) and sim[0][3][6] == LOST and sim[1][3][:3] == (1, 8, 1) and sim[1][3][5] == 8, slots=16)
case("mask_65536_slots_half_live", "the largest table at its limit: 32768 live, one more lost",
     [([request(sid(k), 0) for k in range(32769)], [message(sid(32767)), message(sid(32768))], [], 0)],
     lambda sim: sim[0][3][0] == 32768 and sim[0][3][6] == LOST and sim[0][3][1:3] == (1, 1), slots=65536)
case("expired_by_stream_from_scattered_slots", "the newly expired are listed in no order and ranked by stream",
     [([request(cluster_id(k % 16, (k * 7) % 5), 0, timeout=1) for k in range(40)], [], [], 0), ([], [message(cluster_id(3, 0))], [], 5)],
     lambda sim: [d[2] for d in sim[1][2]] == sorted(d[2] for d in sim[1][2]) and len(sim[1][2]) == sim[0][3][0] > 30
     and sim[1][0][0][6] >> 8 & 0xff == EXPIRED_MSG, slots=128)
# ---- the 4097 keys ------------------------------------------------------------------------------------------------------------------------
case("keys_first_last_and_orphans", "methods 0 and 4095 and the orphans: the scan's first and last trip over the keys",
     [([request(1, 0), request(3, 4095)], [message((1, 3, 5)[i % 3], length=i) for i in range(300)], [], 0)],
     lambda sim: sim[0][1][:2] == [0, 100] and sim[0][1][4095:] == [100, 200, 300] and KEYS == 4097, nmethods=4096)
case("keys_257_methods", "one method more than a trip of the scan over the keys holds",
     [([request(sid(k), k) for k in range(257)], [message(sid(256 - (i % 257))) for i in range(514)], [], 0)],
     lambda sim: sim[0][1] == [2 * m for m in range(258)] + [514] and [r[7] for r in sim[0][0]] == [0, 1] * 257, slots=1024, nmethods=257)


def by_id(cid):
    return next(c for c in CASES if c["id"] == cid)


def rows(c):
    return sum(len(s[0]) + len(s[1]) + len(s[2]) for s in c["steps"])


def emu_subset():
    """the cases small enough for the emulator: at most EMU_MAX rows in all their tables"""
    return [c["id"] for c in CASES if rows(c) <= EMU_MAX]


def simulate(c):
    """the case through the model alone -> [(dispatch, segments, done, result, error) per step]"""
    m, out = CallsModel(c["slots"], c["nmethods"]), []
    for reqs, msgs, events, now in c["steps"]:
        out.append(m.step([r[0] for r in reqs], [r[1] for r in reqs], list(msgs), list(events), now, BIG, BIG))
    return out


def check_cases():
    same(len({c["id"] for c in CASES}), len(CASES), "case ids are unique")
    for c in CASES:
        same(bool(c["wit"](simulate(copy.deepcopy(c)))), True, "the witness of %s (%s)" % (c["id"], c["edge"]))


def run_case(g, c):
    from tests.h2_calls_lib import CH
    h = CH(g, c["slots"], c["nmethods"])
    for reqs, msgs, events, now in c["steps"]:
        h.step(reqs, msgs, events, now)
    h.close()
