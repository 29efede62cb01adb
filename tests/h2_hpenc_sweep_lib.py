"""The header encoder (k_h2_hpenc_scan / _walk / _emit / _commit and k_h2_links_hpenc_*, csrc/grdma_h2_hpenc.h and
csrc/grdma_h2_hpenc_stage.inc) swept over header lists built from the constants it branches on: 256 occurrences a step of
the walk, 257 staged block places, a grid of 64 x 256 lanes (4 x 256 a link), a ring of 2048 entries, a byte ring of 65536,
the prefix widths 4 / 5 / 6 / 7, 61 static entries, 32 bytes of entry overhead (numbers:
profiles/h2_hpenc_sweep.md).

A case is a deterministic script of steps on one HE harness (tests/h2_hpenc_lib.py): ("encode", lists[, caps]),
("encode_raw", (blocks, fields, arena)[, caps]) -- caps: dict(wire_cap=, bw_cap=), a number or ("need", d): what the call
needs plus d -- and ("peer", table, max_frame).  The reference is tests/h2_hpenc_model.HpencModel; HE.encode compares the
whole wire arena with its fill, the block-wire table, the result block, the table dump and the counters exactly.  Nothing
here has a tolerance.

Every case names the edge it is there for, and a witness -- computed from the model alone (simulate) -- shows that the
case reaches it; check_cases() runs them all.  pytest rewrites no `assert` in a helper module: checks go through `same`.

The commit stage lists at most 2048 jobs (one per live entry a call inserted), fewer than the 16384 lanes of the single
form's grid: k_h2_hpenc_commit cannot stride on the device.  A link's share is 4 x 256 = 1024 lanes, so through the batch
call k_h2_links_hpenc_commit takes its loop's second trip on the device in family 5 (1771 and 1942 surviving insertions
in a call at table 65536); under the emulator, where the grids are 2 x 256 lanes, both forms take further trips there.

The many-link form (run_links) puts the same cases through h2dev.encode_batch: step k of every case of a family that has
a step k is one batch call of at most 256 links."""
import copy
import functools

from tests.h2_device_lib import same
from tests.h2_hpack_data import STATIC
from tests.h2_hpenc_lib import FULL_COLLISION, NAME_COLLISION, by_bits, fill
from tests.h2_hpenc_model import (BAD_INPUT, BYTES, CHUNK, ERR_FIELD_RANGE, ERR_LENGTH, ERR_STREAM, ERR_STRING, RING, ByteRing, HpencModel,
                                  enc_int, enc_str, full_hash, huffman_len, live, name_hash, pack, trace)

FAMILIES = ("01", "02", "03", "04", "05", "06", "07", "08", "09", "10", "11")
GRID, LINK_GRID = 64 * 256, 4 * 256  # H2HE_GRID x H2HE_THREADS, H2HE_LINK_GRID x H2HE_THREADS
LINKS_MAX = 256                      # GRDMA_H2_BATCH_MAX
RAW = b"\x01"                        # a byte whose code has 23 bits: strings of it go raw
# cases that were the only ones to catch a change of the mutation table (profiles/h2_hpenc_sweep.md)
CAUGHT_ALONE = ["05_size_update_evicts_across_slot_0_after_2100", "06_three_entries_past_half", "06_equal_hashes_in_the_ring_and_in_the_arena"]
# Where nghttp2 refuses a block the model writes, because of a limit of its own: case id -> the reason.  No entry may cover
# a case where the two disagree on the bytes of a block both accept.
NGHTTP2_DIFFERS = {}

CASES = []


def case(fam, name, edge, key, steps, wit, table=4096, max_frame=16384):
    """key: the edge's kind within the family (emu_subset takes the smallest case of each); wit(sim) -> truth, sim =
    simulate(c): a dict per step"""
    CASES.append(dict(id="%s_%s" % (fam, name), fam=fam, edge=edge, key=key, steps=steps, wit=wit, table=table, max_frame=max_frame))


# ---- builders ---------------------------------------------------------------------------------------------------------
def enc(lists, **caps):
    return ("encode", lists, caps) if caps else ("encode", lists)


def one(fs, stream=1, flags=0):
    return enc([(stream, flags, list(fs))])


def hinted(fs, hint):
    return [(f[0], f[1], hint) for f in fs]


def e36(k):
    """an entry of 36 bytes"""
    return (b"%03d" % k, b"v", 1)


def pat(n, seed):
    return bytes((seed * 29 + 7 * i + (i >> 8)) % 251 for i in range(n))


def sized(target, more=()):
    """a block whose bytes are `target` long: one raw value, then the fields of `more`"""
    for n in range(target - 12, target):
        fs = [(b"x-f", RAW * n, 2)]
        if len(b"\x00" + enc_str(b"x-f") + enc_str(RAW * n)) == target:
            return fs + list(more)
    raise AssertionError(target)


def coded(n):
    """a string of 'a' (five bits) whose Huffman form is n bytes long"""
    return b"a" * (8 * n // 5)


def after(model_steps, table=4096):
    """the model's table behind the steps (for builders that read entries back), newest first"""
    m = HpencModel(table)
    for st in model_steps:
        if st[0] == "peer":
            m.set_peer(st[1], st[2])
        else:
            m.encode(*pack(st[1]), 1 << 40, 1 << 40)
    return list(m.table.entries)


GET = (b":method", b"GET", 1)


# ---- the model alone ----------------------------------------------------------------------------------------------------
def _cap(spec, need):
    return need if spec is None else need + spec[1] if isinstance(spec, tuple) else spec


@functools.lru_cache(maxsize=None)
def _simulate(cid):
    c = by_id(cid)
    model, ring, out = HpencModel(c["table"], c["max_frame"]), ByteRing(), []
    for st in c["steps"]:
        if st[0] == "peer":
            model.set_peer(st[1], st[2])
            out.append(dict(kind="peer"))
            continue
        raw = pack(st[1]) if st[0] == "encode" else st[1]
        caps = st[2] if len(st) > 2 else {}
        blocks, fields, arena = raw
        ahead = copy.deepcopy(model)
        dry = ahead.encode(blocks, fields, arena, 1 << 40, 1 << 40)
        wire_cap, bw_cap = _cap(caps.get("wire_cap"), dry[2][2] + 8), _cap(caps.get("bw_cap"), dry[2][0] + 1)
        tr = trace(model, blocks, fields, arena) if dry[3] is None else dict(occ=[], steps={}, updates=model.updates())
        head0, ins0, calls0, ringb = ring.head, model.table.inserted, model.stats["calls"], bytes(ring.bytes)
        if caps:
            wire, bw, res, err = model.encode(blocks, fields, arena, wire_cap, bw_cap)
        else:  # (the caps are what the call needs and more: the run above is the call)
            model, (wire, bw, res, err) = ahead, dry
        if err is None:
            ring.commit(model.table, res[3])
        t = model.table
        out.append(dict(kind=st[0], raw=raw, caps=(wire_cap, bw_cap), need=(dry[2][2], dry[2][0]), res=res, err=err, wire=wire, bw=bw,
                        occ=tr["occ"], steps=tr["steps"], updates=tr["updates"], nocc=len(tr["occ"]), head0=head0, head1=ring.head, ins0=ins0,
                        ins1=t.inserted, where=list(ring.where), straddles=ring.straddles(), entries=len(t.entries), size=t.size,
                        max_size=t.max_size, live=live(t), table=list(t.entries[:4]), calls=model.stats["calls"] - calls0, ring0=ringb,
                        stats=dict(model.stats)))
    return out


def simulate(c):
    """-> per step what the model alone says: the call's occurrences (trace), its size updates, insertions and the byte
    ring's head in front and behind, the live entries' ring slots, the ring's layout, the result"""
    return _simulate(c["id"])


def reps(s):
    return [o[1] for o in s["occ"]]


def idxs(s):
    return [o[2] for o in s["occ"]]


def inserters(s, step):
    return [i for i, _, _ in s["steps"].get(step, [])]


def bad(s, code, blk):
    return s["err"] == "invalid" and s["res"][6] == (BAD_INPUT | code << 8 | blk << 32) and s["res"][:5] == (0, 0, 0, 0, 0)


# ---- family 1: occurrences per step (H2HE_CHUNK = 256) ----------------------------------------------------------------------
def fam01():
    for n in (255, 256, 257, 511, 512, 513):
        per = [CHUNK] * (n // CHUNK) + ([n % CHUNK] if n % CHUNK else [])
        case("01", "none_inserting_%d" % n, "one block of %d fields, none inserting (hint 2, no match)" % n, "none", [one(hinted(fill(n), 2))],
             lambda sim, n=n: sim[0]["nocc"] == n and set(reps(sim[0])) == {2} and sim[0]["res"][3] == 0 and sim[0]["occ"][-1][0] == (n - 1) // CHUNK)
        case("01", "all_inserting_%d" % n, "one block of %d distinct inserting fields: a round per occurrence" % n, "all", [one(fill(n))],
             lambda sim, n=n, per=per: sim[0]["res"][3] == n and [len(inserters(sim[0], k)) for k in range(len(per))] == per and sim[0]["res"][4] > 0)
        case("01", "same_inserting_%d" % n, "%d times the same inserting field: occurrence 0 inserts, every other one is patched to index 62" % n,
             "same", [one([(b"x-same", b"value", 1)] * n)],
             lambda sim, n=n: sim[0]["res"][3] == 1 and inserters(sim[0], 0) == [0] and idxs(sim[0])[1:] == [62] * (n - 1) and set(reps(sim[0])[1:]) == {0})
    ins, other = (b"x-ins", b"here", 1), (b"x-ins", b"other", 2)
    for step in (0, 1):
        for slot in (0, 1, 254, 255):
            p, last = step * CHUNK + slot, step * CHUNK + CHUNK - 1
            fs = hinted(fill(3 * CHUNK), 2)
            fs[p] = ins
            names = [q for q in (p + 2, last - 1, last + 3) if q > p]
            fulls = [q for q in (p + 1, last, last + 2) if q > p and q not in names]
            for q in names:
                fs[q] = other
            for q in fulls:
                fs[q] = ins
            case("01", "only_inserter_at_slot_%d_of_step_%d" % (slot, step), "the only inserter is occurrence %d; its full and name-only matches in "
                 "the next slot, at the step's last slot and in the step behind" % p, "slot", [one(fs)],
                 lambda sim, p=p, names=names, fulls=fulls, step=step: sim[0]["res"][3] == 1 and inserters(sim[0], step) == [p]
                 and all(sim[0]["occ"][q][1:3] == (0, 62) for q in fulls) and all(sim[0]["occ"][q][1:3] == (2, 62) for q in names)
                 and any(q // CHUNK == step + 1 for q in fulls) and any(q // CHUNK == step + 1 for q in names)
                 and (p % CHUNK == 255 or any(q // CHUNK == step for q in fulls)))
    case("01", "name_chain_300", "300 occurrences of one name, each a new value: 256 rounds in step 0, the name index always 62 through the patch",
         "chain", [one([(b"x-chain", b"%d" % j, 1) for j in range(300)])],
         lambda sim: len(inserters(sim[0], 0)) == CHUNK and sim[0]["res"][3] == 300 and idxs(sim[0])[1:] == [62] * 299 and idxs(sim[0])[0] == 0)
    fs = [f for j in range(200) for f in ((b"x-alt%d" % j, b"v", 1),) * 2]
    case("01", "inserters_alternating_with_their_matches", "200 inserters, each followed by its own full match", "alternate", [one(fs)],
         lambda sim: sim[0]["res"][3] == 200 and reps(sim[0]) == [1, 0] * 200 and idxs(sim[0])[1::2] == [62] * 200 and len(inserters(sim[0], 1)) == 72)


# ---- family 2: evictions inside a step (tables of 0, 72, 100, 108 bytes) -----------------------------------------------------
def fam02():
    pad = lambda n: hinted(fill(n, b"p"), 2)  # noqa: E731  (occurrences that neither match nor insert)
    for table in (72, 100, 108):
        cap = table // 36
        old, new = [e36(k) for k in range(cap)], [e36(100 + k) for k in range(cap)]
        for name, padn in (("round_%d" % (cap + 1), 0), ("slot_255", CHUNK - 1 - cap)):
            case("02", "full_match_lost_table_%d_%s" % (table, name), "table %d: the oldest entry, a full match from the table in front of the step, is "
                 "evicted by the step's first insertion; its occurrence (%d) inserts in round %d" % (table, cap + padn, cap + 1), "lost_full",
                 [one(old), one(new + pad(padn) + [old[0]])],
                 lambda sim, cap=cap, padn=padn: sim[0]["table"][cap - 1] == (b"000", b"v") and inserters(sim[1], 0) == list(range(cap)) + [cap + padn]
                 and sim[1]["res"][3:5] == (cap + 1, cap + 1), table=table)
        case("02", "full_match_lost_across_a_step_table_%d" % table, "table %d: the evicting insertions are the last occurrences of step 0, the loser "
             "is occurrence 256" % table, "across", [one(old), one(pad(CHUNK - cap) + new + [old[0]])],
             lambda sim, cap=cap: inserters(sim[1], 0) == list(range(CHUNK - cap, CHUNK)) and inserters(sim[1], 1) == [CHUNK], table=table)
    for table in (72, 108):
        cap = table // 36
        x, ev = e36(500), [e36(600 + k) for k in range(cap)]
        case("02", "patched_match_lost_table_%d" % table, "table %d: a match gained through the patch (the field inserted earlier in the step) is lost "
             "to the %d insertions that follow; the occurrence inserts again" % (table, cap), "patch_lost", [one([x, x] + ev + [x])],
             lambda sim, cap=cap: reps(sim[0]) == [1, 0] + [1] * (cap + 1) and idxs(sim[0])[1] == 62 and sim[0]["res"][3] == cap + 2, table=table)
        case("02", "patched_match_lost_across_a_step_table_%d" % table, "the same with the first insertion at occurrence 254 and the evicting ones from 255 on",
             "across", [one(pad(CHUNK - 2) + [x] + ev + [x])],
             lambda sim, cap=cap: inserters(sim[0], 0) == [254, 255] and inserters(sim[0], 1) == list(range(CHUNK, CHUNK + cap)), table=table)
    p, q = (b"nnn", b"1", 1), (b"nnn", b"2", 1)
    case("02", "name_match_lost", "table 72: both entries carry the field's name; both are evicted in front of it in the step: no older entry is taken, "
         "the name goes literal", "name_lost", [one([p, q]), one([e36(1), e36(2), (b"nnn", b"9", 2), (b"nnn", b"8", 1)])],
         lambda sim: sim[1]["occ"][2][1:3] == (2, 0) and sim[1]["occ"][3][1:3] == (1, 0) and sim[0]["entries"] == 2, table=72)
    case("02", "full_match_lost_name_match_stays", "table 72: the full match is the older entry, the name match the newer one: the first is evicted, the "
         "occurrence inserts and names the second", "name_lost", [one([p, q]), one([e36(1), p])],
         lambda sim: sim[1]["occ"][1][1:3] == (1, 63) and sim[1]["res"][3:5] == (2, 2), table=72)
    a = (b"abc", b"v", 1)
    for d, what in ((0, "exactly the table size"), (1, "the table size + 1")):
        big = (b"abc", b"y" * (100 - 32 - 3 + d), 1)
        case("02", "entry_of_%s" % what.replace(" ", "_").replace("+", "plus"), "table 100: an entry of %s in mid-step: the table empties, every match behind "
             "it is gone; its own name reference (index 63) stands (RFC 7541 4.4)" % what, "oversize",
             [one([a, e36(7)]), one([a, big, a, a, e36(7)])],
             lambda sim, d=d: sim[1]["occ"][1][1:] == (1, 63, True, 2, d == 0) and reps(sim[1]) == [0, 1, 1, 0, 1] and sim[1]["occ"][2][2] == (62 if d == 0 else 0)
             and sim[1]["entries"] == 2, table=100)
    for n in (256, 600):
        case("02", "%d_inserters_at_table_100" % n, "table 100: %d distinct entries of 36 bytes: every round from the third on evicts" % n, "all_evict",
             [one([e36(k) for k in range(n)])],
             lambda sim, n=n: sim[0]["res"][3:5] == (n, n - 2) and all(o[4] == 1 for o in sim[0]["occ"][2:]) and len(inserters(sim[0], 0)) == CHUNK, table=100)
    case("02", "table_0_257_fields", "table 0: 257 inserting fields insert nothing", "table0", [one(fill(257))],
         lambda sim: sim[0]["res"][3:6] == (0, 0, 0) and set(reps(sim[0])) == {1} and sim[0]["nocc"] == 257 and not any(o[5] for o in sim[0]["occ"]), table=0)


# ---- family 3: blocks per step (257 block places staged a step) ---------------------------------------------------------------
def fam03():
    st = [GET, (b":scheme", b"https", 1)]
    for r in (0, 1, 2):
        for n in (255, 256, 257, 258, 513):
            case("03", "%d_blocks_of_%d" % (n, r), "%d blocks of %d fields" % (n, r), "run%d" % r,
                 [enc([(2 * k + 1, k & 1, st[:r]) for k in range(n)])],
                 lambda sim, n=n, r=r: sim[0]["res"][:2] == (n, n) and sim[0]["nocc"] == n * r and len(sim[0]["wire"]) == n * (9 + r))
    e = (b"x-e", b"1", 1)
    for k in (0, 255, 256):
        for run in (255, 256, 257, 258, 600):
            front = [(1, 0, [GET] * k)] if k else []
            case("03", "%d_empty_blocks_from_occurrence_%d" % (run, k), "a run of %d empty blocks with %d occurrences in front (%s) and a block of three "
                 "fields behind" % (run, k, "one block" if k else "the run is the call's start"), "empties%d" % k,
                 [enc(front + [(3 + 2 * j, 0, []) for j in range(run)] + [(9999, 1, [e, e, (b"x-e", b"2", 2)])])],
                 lambda sim, k=k, run=run: sim[0]["nocc"] == k + 3 and sim[0]["res"][0] == run + 1 + (1 if k else 0) and sim[0]["occ"][k][1:3] == (1, 0)
                 and sim[0]["occ"][k + 1][1:3] == (0, 62) and sim[0]["occ"][k + 2][1:3] == (2, 62) and sim[0]["bw"][-1][1] == 9 + 8 + 1 + 3)
    x = lambda k: (2 * k + 1, 0, [GET, (b"x-b", b"%d" % k, 1)])  # noqa: E731
    for name, lists in (("first", [(1, 0, []), x(1), x(2)]), ("last", [x(0), x(1), (5, 1, [])]), ("consecutive", [x(0), (3, 0, []), (5, 0, []), x(3)])):
        case("03", "empty_block_%s" % name, "an empty block: " + name, "empty", [enc(lists)],
             lambda sim, lists=lists: [b[1] == 9 for b in sim[0]["bw"]] == [not fs for _, _, fs in lists] and sim[0]["res"][0] == len(lists)
             and sim[0]["nocc"] == sum(len(fs) for _, _, fs in lists))
    empties = [(2 * k + 1, k & 1, []) for k in range(300)]
    case("03", "300_empty_blocks", "a call of 300 empty blocks", "all_empty", [enc(empties)],
         lambda sim: sim[0]["res"][:3] == (300, 300, 2700) and sim[0]["nocc"] == 0)
    case("03", "300_empty_blocks_with_a_size_update", "a call of 300 empty blocks, a size update pending: block 0 carries it", "all_empty",
         [one([e]), ("peer", 100, 16384), enc(empties), one([e])],
         lambda sim: sim[2]["res"][:3] == (300, 300, 2702) and sim[2]["updates"] == [100] and sim[2]["bw"][0][1] == 11 and sim[2]["res"][4] == 0
         and sim[3]["occ"][0][1] == 0)
    blocks, fields, arena = pack([(2 * k + 1, 0, [(b"x-d", b"%d" % (k % 3), 1), GET, (b"x-d", b"%d" % k, 2)]) for k in range(6)])
    blocks = [(2 * k + 1, b[1], b[2], b[3]) for k, b in enumerate(reversed(blocks))]
    case("03", "first_field_descends", "six blocks whose first_field descends: block order, not field order, is wire order", "descend",
         [("encode_raw", (blocks, fields, arena))],
         lambda sim: [b[1] for b in sim[0]["raw"][0]] == [15, 12, 9, 6, 3, 0] and reps(sim[0]) == [1, 0, 2] * 3 + [0] * 9
         and sim[0]["res"][3] == 3 and sim[0]["table"][0] == (b"x-d", b"0"))
    blocks, fields, arena = pack([(1, 0, [(b"x-u", b"%d" % j, 1) for j in range(9)])])
    case("03", "fields_no_block_references", "nine fields, the two blocks take fields 1..2 and 6..7", "unreferenced",
         [("encode_raw", ([(1, 1, 2, 0), (3, 6, 2, 0)], fields, arena))],
         lambda sim: sim[0]["nocc"] == 4 and sim[0]["res"][3] == 4 and sim[0]["table"] == [(b"x-u", b"7"), (b"x-u", b"6"), (b"x-u", b"2"), (b"x-u", b"1")])
    blocks, fields, arena = pack([(1, 0, [GET, (b"x-s", b"shared", 1), (b"x-s", b"other", 2)])])
    case("03", "300_blocks_over_three_fields", "300 blocks over the same three fields: 900 occurrences over 3 fields, more than a fresh occurrence "
         "table of 128 holds: one run is refused, the repeat is exact", "shared", [("encode_raw", ([(2 * k + 1, 0, 3, 0) for k in range(300)], fields, arena))],
         lambda sim: sim[0]["nocc"] == 900 and sim[0]["res"][3] == 1 and sim[0]["calls"] == 1 and reps(sim[0])[:6] == [0, 1, 2, 0, 0, 2])
    blocks, fields, arena = pack([(1, 0, [(b"x-o", b"%d" % (j % 8), 1) for j in range(64)])])
    for extra, name in ((0, "fits"), (1, "overflows")):
        bl = [(1, 0, 64, 0), (3, 0, 64, 0)] + [(5, 63, 1, 0)] * extra
        case("03", "occurrences_nfields_plus_%d" % (64 + extra), "64 fields, %d occurrences (nfields + %d): the occurrence table is grown to nfields + 64 "
             "in front of the call, and 64 + 64 = 128 is a capacity h2_grow's doubling from 64 lands on exactly, so on a fresh encoder %s; the second "
             "call runs on the encoder that has grown" % (128 + extra, 64 + extra, "it fits" if not extra else "one run is refused (H2HE_OVER_SCRATCH) "
                                                           "and the repeat is exact: the call counts once, its eight insertions once.  No counter "
                                                           "shows the refused run: that it happens rests on row S of the mutation table "
                                                           "(profiles/h2_hpenc_sweep.md), to be run again when h2_grow or the + 64 changes"), name,
             [("encode_raw", (bl, fields, arena)), ("encode_raw", (bl, fields, arena))],
             lambda sim, extra=extra: sim[0]["nocc"] == 128 + extra and sim[0]["calls"] == 1 and sim[0]["res"][3] == 8 and sim[1]["calls"] == 1
             and sim[1]["res"][3] == 0 and sim[1]["stats"]["calls"] == 2 and sim[1]["stats"]["inserted"] == 8)


# ---- family 4: the grid (64 x 256 lanes; 4 x 256 a link) ----------------------------------------------------------------------
def fam04():
    def fs_of(n, every):
        return [(b"x-g%d" % j, b"v", 1) if every and j % every == 0 else GET for j in range(n)]

    for n, key in ((16383, "grid"), (16384, "grid"), (16385, "grid"), (32769, "grid"), (1023, "link"), (1024, "link"), (1025, "link")):
        lanes = GRID if key == "grid" else LINK_GRID
        case("04", "%d_static_fields" % n, "one block of %d static full matches: %d lanes, the scan's and the emit's loop take %d trips" %
             (n, lanes, -(-n // lanes)), key, [one(fs_of(n, 0))],
             lambda sim, n=n: sim[0]["nocc"] == n and len(sim[0]["wire"]) == n + 9 * (-(-n // 16384)) and sim[0]["res"][3] == 0)
        case("04", "%d_fields_every_97th_inserts" % n, "the same, every 97th field an inserter", key + "_ins", [one(fs_of(n, 97))],
             lambda sim, n=n: sim[0]["nocc"] == n and sim[0]["res"][3] == -(-n // 97) and sim[0]["occ"][97 * ((n - 1) // 97)][3])
    case("04", "16385_blocks_of_one_field", "16385 blocks of one field: emit's loop over the blocks takes its second trip", "blocks",
         [enc([(2 * k + 1, k & 1, [GET]) for k in range(16385)])],
         lambda sim: sim[0]["res"][:3] == (16385, 16385, 163850) and sim[0]["nocc"] == 16385)


# ---- family 5: ring slots (2048) ---------------------------------------------------------------------------------------------------
def fam05():
    ent = lambda a, b: [(b"r", b"%d" % j, 1) for j in range(a, b)]  # noqa: E731
    for table in (4096, 65536):
        for total in (RING, 2 * RING):
            n = total + 52
            steps = [one(ent(0, n))]
            alive = hinted(after(steps, table), 2)
            wit = lambda sim, n=n, total=total: (sim[-1]["ins1"] == n and sim[-1]["live"][-1][0] < total <= sim[-1]["live"][0][0]  # noqa: E731
                                                 and sim[-1]["live"][0][1] == 51 and sim[-1]["live"][-1][1] > 51 and sim[-1]["res"][3] == 0
                                                 and idxs(sim[-1])[-sim[-1]["entries"]:] == list(range(62, 62 + sim[-1]["entries"])) and sim[-1]["entries"] > 100)
            case("05", "%d_insertions_in_one_call_table_%d" % (n, table), "table %d: %d insertions in one call, every live entry read back by full "
                 "match in the same call and in the next: live entries on both sides of slot 0" % (table, n), "wrap%d" % total,
                 [enc([(1, 0, ent(0, n)), (3, 0, alive)]), one(alive)], wit, table=table)
            third = n // 3 + 1
            case("05", "%d_insertions_across_calls_table_%d" % (n, table), "the same across three calls", "wrap%d" % total,
                 [one(ent(k * third, min(n, (k + 1) * third))) for k in range(3)] + [one(alive)], wit, table=table)
    # a size update's evictions at wrapped slots: entries of unequal sizes stand on both sides of slot 0, then the peer
    # lowers its table: the update in front of the next block evicts across the seam (`(ins - cnt) & mask` of the updates)
    uneq = lambda n: [(b"u", (b"%d" % j) * (1 + j % 3), 1) for j in range(n)]  # noqa: E731
    for total in (RING, 2 * RING):
        n = total + 52
        steps = [one(uneq(n)), ("peer", 150, 16384)]
        left = hinted(after(steps + [one([GET])]), 2)
        case("05", "size_update_evicts_across_slot_0_after_%d" % n, "%d insertions of unequal sizes leave live entries on both sides of slot 0; the "
             "peer lowers its table to 150: the size update evicts entries at slots below 2048 and from 0 on, what is left is read back" % n,
             "update%d" % total, steps + [one(left + [(b"u", b"new", 1)] + left[:1])],
             lambda sim, n=n, total=total, left=left: sim[0]["live"][-1][0] < total <= sim[0]["live"][0][0] - len(left) and sim[2]["updates"] == [150]
             and 0 < len(left) < 5 and sim[2]["res"][3] == 1 and sim[2]["res"][4] >= sim[0]["entries"] - len(left) > 50
             and idxs(sim[2])[:len(left)] == list(range(62, 62 + len(left))) and sim[2]["occ"][len(left)][4] > 0 and sim[2]["size"] <= 150)
    # the most entries the rules allow: identical fields index, so entries are distinct: one of 32 bytes, 512 of 33, then 34
    cand = [(b"", b"", 1)] + [(b"", bytes([c]), 1) for c in range(256)] + [(bytes([c]), b"", 1) for c in range(256)]
    cand += [(bytes([a]), bytes([b]), 1) for a in range(0x61, 0x67) for b in range(256)]
    m, most = HpencModel(65536), []
    m.encode(*pack([(1, 0, [GET])]), 1 << 40, 1 << 40)
    for f in cand:  # (as long as the model's table takes one more without an eviction)
        if m.table.size + 32 + len(f[0]) + len(f[1]) > m.table.max_size:
            break
        m.table.field(*f)
        most.append(f)
    same((m.table.evicted, len(m.table.entries)), (0, len(most)), "the most entries: none evicted, all distinct")
    case("05", "the_most_entries", "table 65536: %d distinct entries of 32, 33 and 34 bytes, the most the rules allow (a 2048th would need 2048 x 32 "
         "bytes and identical fields index): the ring is never full; the oldest, the newest and every 64th are read back, then one more insertion evicts "
         "the entry of 32 bytes" % len(most), "most",
         [one([GET]), one(most), one(hinted(most[::64] + [most[-1]], 2) + [(b"zz", b"z", 1), (b"", b"", 2)])],
         lambda sim: sim[1]["entries"] == sim[1]["res"][3] == 1 + 512 + 1429 and sim[1]["entries"] < RING and sim[1]["res"][4] == 0
         and sim[1]["size"] + 34 > 65536 and idxs(sim[2])[0] == 62 + 1941 and sim[2]["res"][3:5] == (1, 1) and sim[2]["occ"][-1][1:3] == (2, 62 + 1 + 1941 - 256),
         table=65536)
    case("05", "empty_name_and_empty_value_as_entries", "entries with an empty name, an empty value and both", "empty_strings",
         [one([(b"", b"", 1), (b"", b"", 1), (b"", b"x", 1), (b"y", b"", 1), (b"y", b"", 0), (b"", b"x", 2), (b"y", b"z", 2)])],
         lambda sim: reps(sim[0]) == [1, 0, 1, 1, 0, 0, 2] and idxs(sim[0]) == [0, 62, 62, 0, 62, 63, 62] and sim[0]["size"] == 32 + 33 + 33)


# ---- family 6: the byte ring (65536) and `fresh` --------------------------------------------------------------------------------
def fam06():
    # sixteen calls insert one entry of 2000 + 2000 string bytes each (table 4096 holds one): the head stands at 64000
    lead = [one([(pat(2000, 2 * k), pat(2000, 2 * k + 1), 1)]) for k in range(16)]
    for what, nl, vl, where in (("name_across", 2000, 2000, "name"), ("name_ends_at_65536", 1536, 0, None), ("value_across", 1000, 3000, "value"),
                                ("seam_at_65536", 1536, 2000, "between")):
        nm, v = pat(nl, 40), pat(vl, 41)
        case("06", what, "the seventeenth entry stands at offset 64000 of the byte ring (%d + %d bytes): %s; found by full match and by name in the next "
             "call, named by the insertion that evicts it in the one behind" % (nl, vl, what.replace("_", " ")), "straddle",
             lead + [one([(nm, v, 1)]), one([(nm, v, 2), (nm, b"short", 2)]), one([(nm, b"x" * 2000, 1), (nm, b"x" * 2000, 0)])],
             lambda sim, where=where, nl=nl: sim[16]["head0"] == 64000 and sim[16]["where"][0][:2] == (64000, nl)
             and (sim[16]["straddles"] == [(62, where)] if where else 64000 + nl == BYTES and not sim[16]["straddles"])
             and [o[1:3] for o in sim[17]["occ"]] == [(0, 62), (2, 62)] and [o[1:3] for o in sim[18]["occ"]] == [(1, 62), (0, 62)]
             and sim[18]["res"][3:5] == (1, 1))
    nl, vl = 30000, 65536 - 32 - 30000
    big = (pat(nl, 5), pat(vl, 6), 1)
    case("06", "one_entry_of_65504_bytes_then_its_name", "table 65536: one entry of 65504 string bytes, matched in the next call, then named by the "
         "insertion that evicts it: the new name lies across 65536", "fill", [one([big]), one([big]), one([(big[0], b"v", 1), (big[0], b"v", 2)])],
         lambda sim: sim[0]["size"] == 65536 and sim[0]["head1"] == 65504 and sim[1]["occ"][0][1:3] == (0, 62) and sim[2]["res"][3:5] == (1, 1)
         and sim[2]["straddles"] == [(62, "name")] and sim[2]["occ"][0][1:3] == (1, 62), table=65536)
    case("06", "one_entry_of_65504_bytes_then_a_small_one", "the same entry, then a small insertion in a later call: its strings stand behind the big one's",
         "fill", [one([big]), one([(b"small", b"one", 1), (b"small", b"one", 1)]), one([(b"small", b"one", 2)])],
         lambda sim: sim[0]["head1"] == 65504 and sim[1]["res"][3:5] == (1, 1) and sim[1]["where"] == [(65504, 5, 3)] and sim[2]["occ"][0][1:3] == (0, 62),
         table=65536)
    three = [(pat(8000, 1), pat(12000, 2), 1), (pat(12000, 3), pat(8000, 4), 1), (pat(5000, 5), pat(5000, 6), 1)]
    case("06", "three_entries_past_half", "table 65536: entries of 20000, 20000 and 10000 string bytes from three calls are alive together; all found by "
         "full match and by name", "half", [one([f]) for f in three] + [one(hinted(three, 2) + [(f[0], b"v", 2) for f in three])],
         lambda sim: sim[2]["where"] == [(40000, 5000, 5000), (20000, 12000, 8000), (0, 8000, 12000)] and idxs(sim[3]) == [64, 63, 62] * 2, table=65536)
    fs = [(pat(2000, 50 + k), pat(2000, 60 + k), 1) for k in range(3)]
    case("06", "inserted_and_evicted_in_one_call", "table 4096: three entries of 4000 string bytes in one call: two are inserted and evicted in it and take "
         "no bytes of the ring", "no_bytes", [one([(b"first", b"entry", 1)]), one(fs), one(hinted(fs[2:], 2))],
         lambda sim: sim[1]["res"][3:5] == (3, 3) and sim[1]["head0"] == 10 and sim[1]["head1"] == 4010 and sim[2]["occ"][0][1:3] == (0, 62))
    a, b = (b"x-prev-entry", b"value-of-prev", 1), (b"y-this-entry", b"value-of-this", 1)
    blocks, fields, arena = pack([(1, 0, [b] + hinted(fill(CHUNK - 1, b"q"), 2) + [hinted([a], 2)[0], hinted([b], 2)[0], (a[0], b"n", 2), (b[0], b"n", 2)])])
    case("06", "fresh_boundary", "the previous call's last entry (its strings in the byte ring at 0) and this call's first (its strings in the arena at "
         "0) are both matched from the table in front of the call's second step: at either offset the arena and the ring hold different bytes", "fresh",
         [one([a]), ("encode_raw", (blocks, fields, arena))],
         lambda sim: sim[0]["where"] == [(0, 12, 13)] and [o[:3] for o in sim[1]["occ"][CHUNK:]] == [(1, 0, 63), (1, 0, 62), (1, 2, 63), (1, 2, 62)]
         and sim[1]["occ"][0][1:3] == (1, 0) and sim[1]["ins0"] == 1 and sim[1]["res"][3] == 1
         and sim[1]["raw"][1][0][:2] == (0, 12) and sim[1]["ring0"][0:12] == a[0] != sim[1]["raw"][2][0:12] and sim[1]["ring0"][12:25] == a[1] != sim[1]["raw"][2][12:25])
    (n1, v1), (n2, v2) = FULL_COLLISION
    c1, c2 = NAME_COLLISION
    case("06", "equal_hashes_in_the_ring_and_in_the_arena", "two fields of one full hash and two names of one name hash: against entries in the byte "
         "ring, and against entries of the same step in the arena, the bytes decide", "collision",
         [one([(n1, v1, 1), (c1, b"v", 1)]), one([(n2, v2, 2), (c2, b"v", 2), (n1, v1, 2), (c1, b"v", 2)]),
          one([(n2, v2, 1), (n1, v1, 1), (n2, v2, 1), (c2, b"w", 1), (c1, b"w", 1), (c2, b"w", 1)])],
         lambda sim: [o[1:3] for o in sim[1]["occ"]] == [(2, 63), (2, 0), (0, 63), (0, 62)]
         and [o[1:3] for o in sim[2]["occ"]] == [(1, 63), (0, 64), (0, 62), (1, 0), (1, 64), (0, 63)] and full_hash(n1, v1) == full_hash(n2, v2)
         and name_hash(c1) == name_hash(c2))


# ---- family 7: integers ---------------------------------------------------------------------------------------------------------
def fam07():
    table = fill(200)
    at = lambda v: table[199 - (v - 62)]  # noqa: E731  (the entry at index v behind the filling call)
    for v in (126, 127, 128, 254, 255, 256):
        case("07", "w7_index_%d" % v, "7-bit prefix: the dynamic index %d" % v, "w7", [one(table), one(hinted([at(v)], 2))],
             lambda sim, v=v: sim[1]["occ"][0][1:3] == (0, v) and len(sim[1]["wire"]) == 9 + len(enc_int(v, 7)), table=65536)
    for v in (62, 63, 64, 190, 191, 192):
        case("07", "w6_name_index_%d" % v, "6-bit prefix: the dynamic name index %d" % v, "w6", [one(table), one([(at(v)[0], b"other", 1)])],
             lambda sim, v=v: sim[1]["occ"][0][1:3] == (1, v) and sim[1]["res"][3] == 1, table=65536)
    for v in (142, 143, 144):
        case("07", "w4_name_index_%d" % v, "4-bit prefix: the dynamic name index %d" % v, "w4", [one(table), one([(at(v)[0], b"other", 2 + v % 2)])],
             lambda sim, v=v: sim[1]["occ"][0][1:3] == (2 + v % 2, v), table=65536)
    for v in (15, 16):  # (14 cannot be a name reference: the static entries 8..14 share the name :status, and the lowest index is taken)
        for hint in (2, 3):
            case("07", "w4_static_name_%d_hint%d" % (v, hint), "4-bit prefix: the static name index %d" % v, "w4s", [one([(STATIC[v][0], b"other", hint)])],
                 lambda sim, v=v, hint=hint: sim[0]["occ"][0][1:3] == (hint, v))
    sizes = (30, 31, 32, 158, 159, 160, 16414, 16415, 16416, 65535, 65536)
    e = (b"x-u", b"1", 1)
    for v in sizes:
        case("07", "w5_size_update_%d" % v, "5-bit prefix: a size update to %d" % v, "w5", [one([e]), ("peer", v, 16384), one([e])],
             lambda sim, v=v: sim[2]["updates"] == [v] and sim[2]["max_size"] == v and sim[2]["wire"][9:9 + len(enc_int(v, 5))] == enc_int(v, 5, 0x20))
        if v < 65536:
            case("07", "w5_size_update_%d_then_65536" % v, "lowered to %d from 65536, then raised: two updates, %d the low one" % (v, v), "w5low",
                 [("peer", 65536, 16384), one([e]), ("peer", v, 16384), ("peer", 65536, 16384), one([e])],
                 lambda sim, v=v: sim[4]["updates"] == [v, 65536] and sim[4]["max_size"] == 65536 and sim[1]["updates"] == [65536])
        case("07", "w5_size_update_0_then_%d" % v, "lowered to 0, then raised to %d: two updates, %d the high one" % (v, v), "w5high",
             [one([e]), ("peer", 0, 16384), ("peer", v, 16384), one([e, e])],
             lambda sim, v=v: sim[3]["updates"] == [0, v] and sim[3]["res"][4] == 1 and reps(sim[3]) == [1, 0 if v >= 36 else 1])
    for v in (126, 127, 128, 254, 255, 256, 16510, 16511, 16512):
        for which in ("name", "value"):
            for h in (False, True):
                s = coded(v) if h else RAW * v
                f = (s, b"v", 2) if which == "name" else (b"x-n", s, 2)
                case("07", "%s_length_%d%s" % (which, v, "_huffman" if h else ""), "7-bit prefix: a %s of %d bytes on the wire, %s" %
                     (which, v, "coded" if h else "raw"), "len_huffman" if h else "len_raw", [one([f])],
                     lambda sim, v=v, h=h, s=s, f=f: enc_str(s)[:len(enc_int(v, 7))] == enc_int(v, 7, 0x80 if h else 0) and len(enc_str(s)) == v + len(enc_int(v, 7))
                     and len(sim[0]["wire"]) == 9 * sim[0]["res"][1] + 1 + len(enc_str(f[0])) + len(enc_str(f[1])) and reps(sim[0]) == [2])


# ---- family 8: Huffman ----------------------------------------------------------------------------------------------------------------
def _tie(align, d):
    """a string whose codes end `align` bits behind a byte and whose coded length is its raw length + d"""
    import itertools
    widths = (5, 6, 7, 8, 10, 11, 13)
    for counts in itertools.product(range(5), repeat=len(widths)):
        nbits, n = sum(k * w for k, w in zip(counts, widths)), sum(counts)
        if n > 1 and nbits % 8 == align and (nbits + 7) // 8 == n + d:
            return b"".join(bytes([by_bits(w)]) * k for w, k in zip(widths, counts))
    raise AssertionError((align, d))


def fam08():
    from tests.h2_hpenc_lib import huffman_bits
    for k in range(8):
        strs = [b"0" * k + bytes([s]) + b"0" * 8 for s in range(256)]  # (eight codes of five bits pay for one of thirty)
        for which in ("value", "name"):
            fs = [(b"n", s, 3) if which == "value" else (s, b"v", 3) for s in strs]
            case("08", "every_byte_behind_%d_codes_as_%s" % (k, which), "every byte value behind %d five-bit codes, as never-indexed %ss, all coded: codes "
                 "of every length end at every bit" % (k, which), which, [one(fs)],
                 lambda sim, strs=strs: all(enc_str(s)[0] & 0x80 for s in strs) and sim[0]["nocc"] == 256 and set(reps(sim[0])) == {3})
        for d, name in ((-1, "one_shorter"), (0, "as_long"), (1, "one_longer")):
            s = _tie(k, d)
            case("08", "coded_%s_ending_at_bit_%d" % (name, k), "a string whose coded form is its raw length %+d and ends %d bits behind a byte: %s" %
                 (d, k, "raw" if d > 0 else "coded (the tie goes coded)"), "tie" + name, [one([(s, s, 2), (b"x-t", s, 3)])],
                 lambda sim, s=s, d=d, k=k: huffman_len(s) == len(s) + d and huffman_bits(s) % 8 == k and bool(enc_str(s)[0] & 0x80) == (d <= 0)
                 and sim[0]["wire"].count(enc_str(s)) == 3)
    s30 = bytes([by_bits(30)])
    case("08", "runs_of_30_bit_symbols", "runs of 1..4 symbols of 30 bits, paid for by codes of five: coded", "long",
         [one([(b"x-l", s30 * r + b"0" * (8 * r), 2) for r in (1, 2, 3, 4)] + [(s30 * 3 + b"0" * 24, b"v", 2)])],
         lambda sim: all(enc_str(s30 * r + b"0" * (8 * r))[0] & 0x80 for r in (1, 2, 3, 4)) and sim[0]["nocc"] == 5)
    text = (b"grpc-status: 0, path=/svc.Name/Method?q=1&r=2; trace=0123456789abcdef " * 300)[:20000 - 256] + bytes(range(256))
    case("08", "one_value_of_20000_bytes", "one value of 20000 bytes of mixed symbols, every byte value among them, coded", "big", [one([(b"x-big", text, 2)])],
         lambda sim: len(text) == 20000 and enc_str(text)[0] & 0x80 and sim[0]["res"][1] == 1 and len(sim[0]["wire"]) > 12000)
    case("08", "name_and_value_decide_independently", "a raw name with a coded value, and the reverse", "independent",
         [one([(RAW * 5, b"aaaa", 2), (b"aaaa", RAW * 5, 2)])],
         lambda sim: sim[0]["wire"][9:] == b"\x00\x05" + RAW * 5 + enc_str(b"aaaa") + b"\x00" + enc_str(b"aaaa") + b"\x05" + RAW * 5 and enc_str(b"aaaa")[0] == 0x83)


# ---- family 9: the static table (61 entries) ------------------------------------------------------------------------------------------
def fam09():
    every = [STATIC[i] for i in range(1, 62)]
    names = [n for n, _ in every]
    lowest = [1 + names.index(n) for n in names]
    for hint in (0, 1, 2, 3):
        case("09", "every_static_entry_hint_%d" % hint, "every static entry as a full match at hint %d: %s (%d of them with an empty value)" %
             (hint, "a never-indexed literal under its static name index" if hint == 3 else "indexed", sum(1 for _, v in every if not v)), "full3" if hint == 3 else "full",
             [one(hinted(every, hint))],
             lambda sim, hint=hint: idxs(sim[0]) == (lowest if hint == 3 else list(range(1, 62))) and set(reps(sim[0])) == {3 if hint == 3 else 0}
             and sim[0]["res"][3] == 0 and sum(1 for _, v in every if not v) > 10)
    for hint in (1, 2, 3):
        case("09", "every_static_name_hint_%d" % hint, "every static name with a value of another kind at hint %d: the lowest index of a shared name" % hint,
             "name", [one([(n, b"foreign-%d" % k, hint) for k, n in enumerate(names)])],
             lambda sim, hint=hint: idxs(sim[0]) == lowest and set(reps(sim[0])) == {hint} and sim[0]["res"][3] == (61 if hint == 1 else 0)
             and lowest != list(range(1, 62)))
    for name, f in (("one_byte_shorter", lambda s: s[:-1]), ("one_byte_longer", lambda s: s + b"x"), ("in_another_case", lambda s: s.upper())):
        miss = [(f(n), v, 2) for n, v in every] + [(n, f(v), 2) for n, v in every if v and (n, f(v)) not in every]
        case("09", "near_miss_%s" % name, "every static name, and every static value, %s: nothing static is taken for the name, and no full match" %
             name.replace("_", " "), "miss", [one(miss)],
             lambda sim, miss=miss: idxs(sim[0])[:61] == [0] * 61 and set(reps(sim[0])) == {2} and idxs(sim[0])[61:] == [1 + names.index(n) for n, _, _ in miss[61:]])
    case("09", "dynamic_entry_with_a_static_name", "an entry whose name is static: its full match is dynamic, its name index stays static", "dynamic",
         [one([(b":path", b"/svc/M", 1), (b":path", b"/svc/M", 2), (b":path", b"/other", 2), (b":path", b"/svc/M", 3)])],
         lambda sim: [o[1:3] for o in sim[0]["occ"]] == [(1, 4), (0, 62), (2, 4), (3, 4)])


# ---- family 10: frames (max_frame >= 16384) ----------------------------------------------------------------------------------------------
def fam10():
    table = fill(200)
    # the fields under the cut: an indexed field of three bytes (index 255), then a literal: 00, a Huffman name with a
    # two-byte length, a raw value with a three-byte length
    group = [hinted([table[199 - (255 - 62)]], 2)[0], (b"a" * 400, RAW * 300, 2)]
    glen = 3 + 1 + 2 + 250 + 3 + 300
    for p in list(range(1, 25)) + list(range(glen - 4, glen)):
        case("10", "cut_behind_byte_%d_of_the_fields" % p, "an indexed field of three bytes and a literal (00, a coded name under a two-byte length, a raw "
             "value under a three-byte length), %d bytes: the frame ends behind byte %d of them" % (glen, p), "cut",
             [one(table), one(sized(16384 - p, group))],
             lambda sim, p=p: sim[1]["res"][1] == 2 and sim[1]["bw"][0] == (0, 16384 - p + glen + 18, 2) and sim[1]["occ"][1][1:3] == (0, 255)
             and len(enc_str(b"a" * 400)) == 252 and sim[1]["wire"][9 + 16384 - p:9 + 16384 - p + 3] == enc_int(255, 7, 0x80)[:min(p, 3)] + sim[1]["wire"][9 + 16384:9 + 16384 + 3 - min(p, 3)],
             table=65536)
    for n in (16383, 16384, 16385, 32767, 32768, 32769):
        nfr = -(-n // 16384)
        case("10", "block_of_%d_bytes" % n, "a block of %d bytes: %d frames" % (n, nfr), "length", [enc([(1, 1, sized(n)), (3, 0, [GET])])],
             lambda sim, n=n, nfr=nfr: sim[0]["bw"] == [(0, n + 9 * nfr, nfr), (n + 9 * nfr, 10, 1)] and sim[0]["res"][1] == nfr + 1)
    case("10", "cut_between_two_fields", "the frame ends exactly between two fields", "between", [one(sized(16384, [GET, (b"x-b", b"1", 1)]))],
         lambda sim: sim[0]["res"][1] == 2 and sim[0]["wire"][9 + 16384:9 + 16384 + 10] == b"\x00\x00\x08\x09\x04\x00\x00\x00\x01\x82")
    for name, peers, lead in (("1", [20], 1), ("3", [1000], 3), ("3_and_3", [1000, 2000], 6)):
        case("10", "size_updates_of_%s_bytes_push_the_field_across" % name, "a block of 16384 bytes behind size updates of %d bytes: the updates move its "
             "only field across the cut" % lead, "lead", [one([GET])] + [("peer", v, 16384) for v in peers] + [one(sized(16384))],
             lambda sim, lead=lead, peers=peers: sim[-1]["updates"] == peers and sim[-1]["res"][1] == 2 and sim[-1]["bw"][0][1] == 16384 + lead + 18)
    for mf in (16385, (1 << 24) - 1):
        case("10", "max_frame_%d" % mf, "max_frame %d: a block of 16385 bytes is one frame, one of 40000 bytes %s" % (mf, "three" if mf == 16385 else "one"),
             "max_frame", [one(sized(16385)), one(sized(40000))],
             lambda sim, mf=mf: sim[0]["res"][1] == 1 and sim[1]["res"][1] == -(-40000 // mf), max_frame=mf)
    case("10", "last_block_ends_at_a_frames_end", "the call's last block is 32768 bytes: its second frame is full", "exact_end",
         [enc([(1, 0, [GET]), (3, 0, sized(32768))])], lambda sim: sim[0]["bw"][1] == (10, 32768 + 18, 2) and len(sim[0]["wire"]) == 10 + 32768 + 18)
    case("10", "end_stream_on_the_first_frame_only", "END_STREAM on a block of three frames", "end_stream", [enc([(1, 1, sized(40000)), (3, 0, sized(20000))])],
         lambda sim: sim[0]["res"][1] == 5 and [sim[0]["wire"][o + 4] for o in (0, 9 + 16384, 18 + 32768)] == [1, 0, 4] and sim[0]["wire"][40027 + 4] == 0)
    case("10", "flags_0xff", "flags 0xff give END_STREAM alone", "flags", [enc([(1, 0xff, [GET]), (3, 0xfe, [GET])])],
         lambda sim: sim[0]["wire"][4] == 5 and sim[0]["wire"][14] == 4)
    case("10", "stream_ids_1_and_2p31m1", "the stream ids 1 and 2^31 - 1", "stream", [enc([(1, 0, [GET]), ((1 << 31) - 1, 0, sized(16385))])],
         lambda sim: sim[0]["wire"][15:19] == b"\x7f\xff\xff\xff" and sim[0]["wire"][10 + 9 + 16384 + 5:10 + 9 + 16384 + 9] == b"\x7f\xff\xff\xff")


# ---- family 11: bad input and caps ---------------------------------------------------------------------------------------------------------
def fam11():
    before, good = one([(b"x-before", b"it", 1)]), one([(b"x-before", b"it", 1), (b"x-after", b"it", 1)])
    untouched = lambda sim, code, blk: (bad(sim[1], code, blk) and sim[1]["entries"] == 1 and sim[1]["stats"] == sim[0]["stats"]  # noqa: E731
                                        and sim[2]["err"] is None and reps(sim[2]) == [0, 1])

    def spoil(raw, fi, code):
        blocks, fields, arena = raw
        no, vo, nl, vl = fields[fi]
        fields = list(fields)
        fields[fi] = (no, vo, nl, 1 << 24) if code == ERR_LENGTH else (no, len(arena) - vl + 1, nl, vl)
        return blocks, fields, arena

    ins = lambda k: (b"x-i%d" % k, b"v", 1)  # noqa: E731
    for i in (255, 256, 257):
        raw = spoil(pack([(1, 0, [ins(0), ins(1)] + hinted(fill(298), 2))]), i, ERR_STRING)
        case("11", "bad_field_at_occurrence_%d" % i, "a string past the arena in occurrence %d, behind two insertions" % i, "occurrence",
             [before, ("encode_raw", raw), good], lambda sim: untouched(sim, ERR_STRING, 0))
    five = [(2 * k + 1, 0, [ins(k), (b"x-f", b"%d" % k, 2), GET]) for k in range(5)]
    for a, b, name in ((ERR_LENGTH, ERR_STRING, "length_then_string"), (ERR_STRING, ERR_LENGTH, "string_then_length")):
        raw = spoil(spoil(pack(five), 6, a), 8, b)
        case("11", "two_bad_fields_%s" % name, "two bad fields of different codes in block 2: the first decides", "two",
             [before, ("encode_raw", raw), good], lambda sim, a=a: untouched(sim, a, 2))
    blocks, fields, arena = spoil(pack(five), 4, ERR_STRING)
    b3 = [b if k != 3 else (0,) + b[1:] for k, b in enumerate(blocks)]
    case("11", "bad_field_in_block_1_bad_block_3", "a bad field in block 1, stream 0 in block 3: block 1 decides", "both",
         [before, ("encode_raw", (b3, fields, arena)), good], lambda sim: untouched(sim, ERR_STRING, 1))
    blocks, fields, arena = spoil(pack(five), 10, ERR_LENGTH)
    b1 = [b if k != 1 else (b[0], 14, 3, 0) for k, b in enumerate(blocks)]
    case("11", "bad_block_1_bad_field_in_block_3", "block 1 reaches past the field table, a bad field in block 3: block 1 decides", "both",
         [before, ("encode_raw", (b1, fields, arena)), good], lambda sim: untouched(sim, ERR_FIELD_RANGE, 1))
    blocks, fields, arena = spoil(pack(five), 7, ERR_STRING)
    b2 = [b if k != 2 else (1 << 31,) + b[1:] for k, b in enumerate(blocks)]
    case("11", "bad_block_with_a_bad_field", "block 2 has the stream id 2^31 and a bad field: the block's code decides", "both",
         [before, ("encode_raw", (b2, fields, arena)), good], lambda sim: untouched(sim, ERR_STREAM, 2))
    blocks, fields, arena = spoil(pack(five), 4, ERR_LENGTH)
    skip = [b if k != 1 else (b[0], 3, 1, 0) for k, b in enumerate(blocks)]
    case("11", "bad_field_no_block_references", "a bad field no block references is no error", "unreferenced",
         [before, ("encode_raw", (skip, fields, arena)), good],
         lambda sim: sim[1]["err"] is None and sim[1]["nocc"] == 13 and sim[1]["res"][3] == 5 and sim[2]["err"] is None)
    blocks, fields, arena = spoil(pack([(1, 0, [ins(0), ins(1), ins(2), ins(3)])]), 3, ERR_STRING)
    case("11", "bad_field_through_the_second_sharing_block", "blocks over fields 0..2 and 1..3 share two fields; field 3 is bad: block 1", "shared",
         [before, ("encode_raw", ([(1, 0, 3, 0), (3, 1, 3, 0)], fields, arena)), good], lambda sim: untouched(sim, ERR_STRING, 1))
    blocks, fields, arena = pack([(1, 0, [ins(0), (b"x-end", b"of the arena", 1)])])
    case("11", "string_ends_at_strings_bytes", "a value that ends exactly at strings_bytes", "end",
         [before, ("encode_raw", (blocks, fields, arena)), good],
         lambda sim: sim[1]["err"] is None and sim[1]["raw"][1][1][1] + sim[1]["raw"][1][1][3] == len(sim[1]["raw"][2]) and sim[1]["res"][3] == 2)
    case("11", "string_ends_one_byte_past_strings_bytes", "the same value, the arena one byte shorter", "end",
         [before, ("encode_raw", (blocks, fields, arena[:-1])), good], lambda sim: untouched(sim, ERR_STRING, 0))
    call = [(1, 0, fill(30, b"c")), (3, 1, hinted(fill(30, b"c")[25:], 2) + [(b"x-c", b"w" * 300, 1)])]
    for what in ("wire_cap", "bw_cap"):
        case("11", "%s_one_short_then_exact" % what, "a call with insertions, evictions and a pending pair of size updates: %s one short of what it "
             "needs (nothing is written or committed), then exactly that: the repeat is exact" % what, what,
             [one(fill(20)), ("peer", 50, 16384), ("peer", 400, 16384), enc(call, **{what: ("need", -9 if what == "wire_cap" else -2)}),
              enc(call, wire_cap=("need", -8), bw_cap=("need", -1))],
             lambda sim, what=what: sim[3]["err"] == "capacity" and sim[3]["res"][7] == 1 and sim[3]["stats"] == sim[0]["stats"] and sim[3]["entries"] == 20
             and sim[3]["caps"][what == "bw_cap"] == sim[3]["need"][what == "bw_cap"] - 1 and sim[4]["err"] is None and sim[4]["caps"] == sim[4]["need"]
             and sim[4]["updates"] == [50, 400] and sim[4]["res"][3] > 0 and sim[4]["res"][4] >= 20 and sim[4]["res"][:7] == sim[3]["res"][:7])


for _f in (fam01, fam02, fam03, fam04, fam05, fam06, fam07, fam08, fam09, fam10, fam11):
    _f()
_BY_ID = {c["id"]: c for c in CASES}


def by_id(cid):
    return _BY_ID[cid]


def check_cases():
    """every case's witness, from the model alone -> the cases"""
    same(len(_BY_ID), len(CASES), "case ids are unique")
    for c in CASES:
        same(bool(c["wit"](simulate(c))), True, "case %s reaches its edge (%s)" % (c["id"], c["edge"]))
    return CASES


def size_of(c):
    """the case's occurrences, and a 64th of its string bytes (read off the steps: no model runs)"""
    n = 0
    for st in c["steps"]:
        if st[0] == "encode":
            n += sum(len(fs) + sum(len(f[0]) + len(f[1]) for f in fs) // 64 for _, _, fs in st[1])
        elif st[0] == "encode_raw":
            n += sum(b[2] for b in st[1][0]) + len(st[1][2]) // 64
    return n


def emu_subset():
    """the CPU suite's part: of every family and kind of edge the case with the fewest occurrences, plus every case that
    caught a change of the mutation table alone"""
    best = {}
    for c in CASES:
        k = (c["fam"], c["key"])
        if k not in best or size_of(c) < size_of(best[k]):
            best[k] = c
    out = [c["id"] for c in CASES if best[(c["fam"], c["key"])] is c]
    return out + [t for t in CAUGHT_ALONE if t not in out]


def links_cases(fam, only=None):
    """the cases of a family that go through the batch call (only: of these ids): family 4's are those sized for a
    link's share of the grid"""
    return [c for c in CASES if c["fam"] == fam and (fam != "04" or c["key"].startswith("link")) and (only is None or c["id"] in only)]


def pin_sequence(c):
    """the case for a decoder: [("peer", table size)] where the peer's setting changes, and per committed call ("call",
    the header lists [(stream, end_stream, [(name, value, hint)])], the wire bytes, the table behind the call)"""
    out = []
    model = HpencModel(c["table"], c["max_frame"])
    for st, s in zip(c["steps"], simulate(c)):
        if st[0] == "peer":
            model.set_peer(st[1], st[2])
            out.append(("peer", st[1]))
            continue
        blocks, fields, arena = s["raw"]
        wire, _, _, err = model.encode(blocks, fields, arena, *s["caps"])
        same(wire, s["wire"], "%s: the replay" % c["id"])
        if err is None:
            lists = [(sid, fl & 1, [(bytes(arena[no:no + (nl & 0xffffff)]), bytes(arena[vo:vo + vl]), nl >> 24 & 3) for no, vo, nl, vl in fields[first:first + n]])
                     for sid, first, n, fl in blocks]
            out.append(("call", lists, wire, (list(model.table.entries), model.table.size)))
    return out


# ---- the drivers -----------------------------------------------------------------------------------------------------------------
def run_case(g, c):
    from tests.h2_hpenc_lib import HE
    sim = simulate(c)
    h = HE(g, c["table"], c["max_frame"])
    for k, (st, s) in enumerate(zip(c["steps"], sim)):
        if st[0] == "peer":
            h.set_peer(st[1], st[2])
            continue
        _, _, res = h.encode(raw=s["raw"], wire_cap=s["caps"][0], bw_cap=s["caps"][1])
        same(res, s["res"], "step %d: the harness's model against the case's" % k)
    h.close()


def run_links(g, fam, only=None):
    """the family's cases, one link each, through h2dev.encode_batch: step k of every case that has one in one call"""
    from tests.h2_links_hpenc_lib import HE, encode_batch
    cs = links_cases(fam, only)
    for lo in range(0, len(cs), LINKS_MAX):
        part = cs[lo:lo + LINKS_MAX]
        hs = [HE(g, c["table"], c["max_frame"]) for c in part]
        for k in range(max(len(c["steps"]) for c in part)):
            order, raw, caps = [], {}, {}
            for i, c in enumerate(part):
                if k >= len(c["steps"]):
                    continue
                st = c["steps"][k]
                if st[0] == "peer":
                    hs[i].set_peer(st[1], st[2])
                    continue
                s = simulate(c)[k]
                order.append(i)
                raw[i], caps[i] = s["raw"], s["caps"]
            if not order:
                continue
            _, got = encode_batch(hs, order, raw=raw, caps=caps)
            for i in order:
                same(got[i][2], simulate(part[i])[k]["res"], "%s step %d: the harness's model against the case's" % (part[i]["id"], k))
        for h in hs:
            h.close()
