// The call table (grdma_h2_calls): per-call state of ONE connection in HBM, keyed by stream, joined in every step with
// the step's call records (the metadata reader's), received-message descriptors (the assembler's) and STREAM_CLOSED
// events (the deframer's), all device tables passed by address.  A step writes the messages as one contiguous work list
// per registered method (the dispatch table and its segment words) and a done list (deadlines, closes).  The rules stand
// in include/grdma_amd.h ("Call table"); the sequential reference is tests/h2_calls_model.py.  The table belongs to no
// parser.
//
// The table is rebuilt into the other of two tables in every step (nothing is deleted in place; a call that LEFT stays
// behind as a dead entry until the next rebuild), and the commit is the flip: a step refused for its caps flips nothing.
// Keys hash as everywhere: (id >> 1) & mask, linear probing.  A compare-and-swap settles a SLOT, never an order: every
// order comes from an index (the lowest record per stream, the lowest closing event per stream: atomicMin) or a scan.
//
// Eight launches of fixed shape, whatever the counts.  A workgroup owns a contiguous RUN of the records, of the
// descriptors and of the events (h2c_run), the same in every stage:
//   k_h2_calls_clear   the new table, the per-entry step words, the record-dedup table, the count rows
//   k_h2_calls_claim   a lane per record: would it open a call, is it bad input (atomicMin of record << 8 | code), does
//                      its stream have a live entry (a duplicate); else its stream's slot in the dedup table takes the
//                      lowest record index
//   k_h2_calls_wins    a lane per record: the winner of its stream; the winners of a run are counted (ballot)
//   k_h2_calls_insert  the winners' ranks (the runs in front, a block scan): serial = counter + rank, opened while the
//                      live count allows; the live entries of the old table copied beside them; EXPIRE on insertion,
//                      the newly expired appended to a list (its order is settled later, by stream)
//   k_h2_calls_msgs    the descriptors of a run in order, 256 at a time: lookup and the orphan checks; within a wave
//                      the rank among the lanes of the same entry and of the same method (ballot, a shuffle from the leading lane); the four
//                      waves then take turns adding to the run's count rows (row[run][slot], row[run][key]), so a
//                      descriptor knows how many of its key the run holds in front of it.  The entry's bytes, count
//                      and last descriptor: order-free atomics.  Beside it a lane per event: the lowest LEFT and the
//                      lowest reads-closed event per entry
//   k_h2_calls_cols    a lane per key and per slot: the exclusive prefix down the runs' rows, the key's total; the
//                      closing events that count, per run; the rank by stream of every newly expired entry; the LEFT
//                      entries counted
//   k_h2_calls_finish  one workgroup: the scan over the at most 4097 keys' totals, the totals of the step, bad input or
//                      a cap too small (the result block alone), else the segment words, the counters and the flip
//   k_h2_calls_emit    the dispatch records at segment + rows in front + rank; the done list; the entries made final
// Kernel boundaries are the only agent-scope hand-over.  The bodies stand in csrc/grdma_h2_calls_stage.inc: the same text
// serves the tables of many links in the same eight launches (k_h2_links_calls_*, below).
#ifndef GRDMA_H2_CALLS_H
#define GRDMA_H2_CALLS_H
#include "grdma_h2_meta.h"

#define H2C_THREADS 256
#ifdef GRDMA_WAVE_EMU
#define H2C_GRID 2  // (the emulator runs workgroups one after another)
#else
#define H2C_GRID 64
#endif
#define H2C_NONE 0xffffffffu
#define H2C_KEYS_MAX 4097u     // 4096 methods and the orphans
#define H2C_SLOTS_MAX 65536u
#define H2C_MSGS_MAX (1ull << 20)

enum { H2C_OPENED = 0, H2C_DISPATCHED = 1, H2C_ORPHANS = 2, H2C_DONE = 3, H2C_EXPIRED = 4, H2C_LIVE = 5, H2C_FLAGS = 6, H2C_OVERFLOW = 7 };
enum { H2C_F_BAD_INPUT = 1, H2C_F_LOST = 2 };
enum { H2C_E_STREAM = 1, H2C_E_METHOD = 2 };
enum { H2C_FIRST = 1, H2C_LAST = 2, H2C_COMPRESSED = 4 };
enum { H2C_NO_CALL = 1, H2C_EXPIRED_MSG = 2, H2C_BAD_STATUS = 3, H2C_COMPRESSED_IDENTITY = 4 };
enum { H2C_READS_CLOSED = 1, H2C_LEFT = 2, H2C_DEADLINE = 3 };
// an entry's flags (word bits 8..15); DEAD never leaves the device
enum { H2C_EF_READS_CLOSED = 1u << 8, H2C_EF_EXPIRED = 2u << 8, H2C_EF_DEAD = 0x80u << 8 };
enum { H2C_CLS_NO = 0, H2C_CLS_CAND = 1, H2C_CLS_WIN = 2 };

struct h2c_entry { uint64_t call, deadline, bytes; uint32_t stream, method, messages, word, fin, pad1; };  // 48 bytes; stream 0: empty.  fin: flags the step's last stage adds (word | fin counts)
struct h2c_aux { uint32_t left_at, rc_at, last, nstep, m0, new_exp, pad0, pad1; };  // an entry's words of the step
struct h2c_dd { uint32_t key, rec; };                    // record dedup: the lowest candidate record of a stream
struct h2c_mrec { uint32_t slot, key, rank_s, rank_k; }; // a descriptor as k_h2_calls_msgs leaves it (an orphan: rank_s is the reason)
struct h2c_disp { uint64_t offset, length, call; uint32_t stream, msg, method, word, seq, pad; };  // grdma_h2_dispatch
struct h2c_done { uint64_t call, bytes; uint32_t stream, method, messages, word; };                // grdma_h2_call_done
struct h2c_msg { uint64_t offset, length, seq; uint32_t stream, status, flags, pad; };             // grdma_h2_rx_msg

// one step (the host's words)
struct h2c_call {
  const h2hp_block_out* blocks;
  const h2m_meta_out* meta;
  uint64_t nblocks;
  const h2c_msg* msgs;
  uint64_t nmsgs;
  const grdma_h2_event* ev;
  uint64_t nev;
  uint64_t now;
  h2c_disp* disp;
  uint64_t disp_cap;
  uint32_t* segs;
  h2c_done* done;
  uint64_t done_cap;
  uint32_t* cls;     // one per record
  h2c_dd* dd;        // dd_mask + 1 slots, a power of two >= 2 nblocks
  uint64_t dd_mask;
  h2c_mrec* mrec;    // one per descriptor
};

// the table, resident in HBM
struct h2c_dev {
  h2c_call c;
  // set at create
  h2c_entry* tab[2];
  h2c_aux* aux;        // of the table a step builds
  uint32_t* row_s;     // H2C_GRID rows of `slots` counts
  uint32_t* row_k;     // H2C_GRID rows of H2C_KEYS_MAX counts
  uint32_t* ktot;      // H2C_KEYS_MAX + 1: a key's total, then (finish) its segment's start
  uint32_t* exp_slot;  // slots / 2: the newly expired, then their rank by stream
  uint32_t* exp_rank;
  uint32_t slots, nmethods;
  // state
  uint32_t cur, live, lost, emit_tab;
  uint64_t serial;
  uint64_t st_steps, st_opened, st_msgs, st_bytes, st_orphans, st_done;  // since creation
  // of the step
  unsigned long long bad;  // the first bad record << 8 | code, ~0: none
  uint32_t nexp, nleft, go, pad;
  uint32_t wins[H2C_GRID], closes[H2C_GRID];
  uint64_t wg_bytes[H2C_GRID];
  uint64_t res[8];  // H2C_*
};

namespace {

// the run of n items workgroup w of the nblk that share them takes: [*b0, *b1), a multiple of the workgroup's threads long
__device__ __forceinline__ void h2c_run(uint64_t n, uint32_t w, uint32_t nblk, uint64_t* b0, uint64_t* b1) {
  uint64_t per = (n + nblk - 1u) / nblk;
  per = (per + H2C_THREADS - 1u) / H2C_THREADS * H2C_THREADS;
  const uint64_t lo = per * w, hi = lo + per;
  *b0 = lo < n ? lo : n;
  *b1 = hi < n ? hi : n;
}
// the slot of stream id in a table that is not being written, H2C_NONE: no entry (a dead one is found: the caller looks)
__device__ __forceinline__ uint32_t h2c_find(const h2c_entry* t, uint32_t m, uint32_t id) {
  uint32_t s = (id >> 1) & m;
  for (uint32_t probe = 0; probe <= m; probe++, s = (s + 1u) & m) {
    const uint32_t k = t[s].stream;
    if (k == id) return s;
    if (k == 0) return H2C_NONE;
  }
  return H2C_NONE;
}
// the slot of id in a table under construction: claimed, or found (as h2sw_claim)
__device__ __forceinline__ uint32_t h2c_claim(uint32_t* key0, uint32_t stride_words, uint32_t m, uint32_t id) {
  uint32_t s = (id >> 1) & m;
  for (uint32_t probe = 0; probe <= m; probe++, s = (s + 1u) & m) {
    uint32_t* const p = key0 + (size_t)s * stride_words;
    uint32_t k = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0 && __hip_atomic_compare_exchange_strong(p, &k, id, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return s;
    if (k == id) return s;  // (a failed exchange leaves the winner's key in k)
  }
  return H2C_NONE;
}
// the first three conditions of OPEN: a REQUEST, verdict OK, the block's status byte 0
__device__ __forceinline__ bool h2c_would_open(uint32_t word, uint32_t block_flags) {
  return (word & 0xffu) == H2M_REQUEST && ((word >> 8) & 0xffu) == H2M_OK && ((block_flags >> 8) & 0xffu) == 0;
}
// among the lanes of the wave that are `on`, those with this lane's key: how many lie in front of it, how many there
// are, and whether this is the last of them (every lane calls it: the loop's ballots are the wave's)
__device__ __forceinline__ void h2c_keyed(uint32_t key, bool on, uint32_t lane, uint32_t* rank, uint32_t* tot, bool* last) {
  uint64_t todo = __ballot(on);
  *rank = 0, *tot = 0, *last = false;
  while (todo) {  // (uniform)
    const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
    const uint32_t k = (uint32_t)__shfl((int)key, (int)lead, 64);
    const bool mine = on && key == k;
    const uint64_t same = __ballot(mine);
    if (mine) {
      *rank = (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1ull));
      *tot = (uint32_t)__builtin_popcountll(same);
      *last = (same >> lane) == 1ull;
    }
    todo &= ~same;
  }
}
// a new entry, or a live one copied, goes into the table under construction; EXPIRE as it goes in
__device__ __forceinline__ void h2c_put(h2c_dev* F, h2c_entry* neu, h2c_entry e, uint64_t now) {
  const uint32_t s = h2c_claim(&neu[0].stream, sizeof(h2c_entry) / 4u, F->slots - 1u, e.stream);
  if (s == H2C_NONE) return;  // (at most slots / 2 go in: cannot be)
  uint32_t new_exp = 0;
  if (!(e.word & H2C_EF_EXPIRED) && e.deadline <= now) {
    e.word |= H2C_EF_EXPIRED;
    new_exp = 1;
    const uint32_t at = atomicAdd(&F->nexp, 1u);  // (a place in the list, not an order: k_h2_calls_cols ranks by stream)
    if (at < F->slots / 2u) F->exp_slot[at] = s;
  }
  neu[s].call = e.call, neu[s].deadline = e.deadline, neu[s].bytes = e.bytes;
  neu[s].method = e.method, neu[s].messages = e.messages, neu[s].word = e.word, neu[s].fin = 0, neu[s].pad1 = 0;
  F->aux[s].m0 = e.messages;
  F->aux[s].new_exp = new_exp;
}
// whether event j of the step is a close that writes a record: a STREAM_CLOSED of a stream with an entry, not behind the
// entry's LEFT.  *slot: the entry
__device__ __forceinline__ bool h2c_closes(const h2c_dev* F, const h2c_entry* neu, const grdma_h2_event& e, uint64_t j, uint32_t* slot) {
  if (e.kind != EV_STREAM_CLOSED || e.a > 1u || e.c == 0) return false;
  const uint32_t s = h2c_find(neu, F->slots - 1u, e.c);
  if (s == H2C_NONE) return false;
  *slot = s;
  const uint32_t left_at = F->aux[s].left_at;
  return e.a ? (uint32_t)j == left_at : (left_at == H2C_NONE || (uint32_t)j < left_at);
}

// ---- the eight stages of ONE table: the bodies are csrc/grdma_h2_calls_stage.inc over the whole grid
#define H2C_BLK blockIdx.x
#define H2C_NBLK H2C_GRID
__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_clear(h2c_dev* F) {
  const h2c_call* const C = &F->c;
#define H2C_STAGE 1
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_claim(h2c_dev* F) {
  const h2c_call* const C = &F->c;
#define H2C_STAGE 2
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_wins(h2c_dev* F) {
  const h2c_call* const C = &F->c;
#define H2C_STAGE 3
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_insert(h2c_dev* F) {
  const h2c_call* const C = &F->c;
#define H2C_STAGE 4
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_msgs(h2c_dev* F) {
  const h2c_call* const C = &F->c;
#define H2C_STAGE 5
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_cols(h2c_dev* F) {
  const h2c_call* const C = &F->c;
#define H2C_STAGE 6
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_finish(h2c_dev* F) {
  const h2c_call* const C = &F->c;
  uint64_t* const R = F->res;
#define H2C_STAGE 7
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_emit(h2c_dev* F) {
  const h2c_call* const C = &F->c;
#define H2C_STAGE 8
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
#undef H2C_BLK
#undef H2C_NBLK

// ---- the eight stages over a table of L <= H2C_LINKS_MAX links: eight launches however many links.  Every link has a
// call table of its own (its state is per connection, as the header encoder's): an entry of the link table is that
// table, its step's words and its eight result words, the latter two in the batch block of the host call (one copy up,
// one copy down for all links), so F->c of no table is touched, and bad input and a cap overflow stay with their link.
// Link l owns the workgroups [l * H2C_LINK_GRID, (l + 1) * H2C_LINK_GRID) in seven stages and workgroup l of the finish
// launch.  A table's count rows, wins, closes and wg_bytes are sized for H2C_GRID runs: a link's fewer runs use the first
// H2C_LINK_GRID of them, so single and batch steps may alternate on one table and no table needs memory for the batch.
#define H2C_LINKS_MAX 256  // (= GRDMA_H2_BATCH_MAX, include/grdma_amd.h)
#ifdef GRDMA_WAVE_EMU
#define H2C_LINK_GRID 2
#else
#define H2C_LINK_GRID 4    // (256 links: 1024 workgroups, four to a compute unit)
#endif
static_assert(H2C_LINK_GRID <= H2C_GRID, "a link's runs use a table's rows, which are sized for H2C_GRID runs");
struct h2c_link {
  h2c_dev* F;            // the link's table
  const h2c_call* call;  // in the batch block
  uint64_t* res;         // the item's eight words in the batch block: H2C_*
};
// (the table is written by the host in front of the launch and only read on the device: constant memory, as H2M_ENTRY)
#ifdef GRDMA_WAVE_EMU
#define H2C_ENTRY(tab, l) ((tab)[l])
#else
#define H2C_ENTRY(tab, l) (((const __attribute__((address_space(4))) h2c_link*)(tab))[l])
#endif

#define H2C_BLK (blockIdx.x % H2C_LINK_GRID)
#define H2C_NBLK H2C_LINK_GRID
#define H2C_OF(l)                                             \
  if ((l) >= nlinks) return; /* (uniform in the workgroup) */ \
  h2c_dev* const F = H2C_ENTRY(tab, l).F;                     \
  const h2c_call* const C = H2C_ENTRY(tab, l).call;
__global__ __launch_bounds__(H2C_THREADS) void k_h2_links_calls_clear(const h2c_link* __restrict__ tab, uint32_t nlinks) {
  H2C_OF(blockIdx.x / H2C_LINK_GRID)
#define H2C_STAGE 1
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_links_calls_claim(const h2c_link* __restrict__ tab, uint32_t nlinks) {
  H2C_OF(blockIdx.x / H2C_LINK_GRID)
#define H2C_STAGE 2
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_links_calls_wins(const h2c_link* __restrict__ tab, uint32_t nlinks) {
  H2C_OF(blockIdx.x / H2C_LINK_GRID)
#define H2C_STAGE 3
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_links_calls_insert(const h2c_link* __restrict__ tab, uint32_t nlinks) {
  H2C_OF(blockIdx.x / H2C_LINK_GRID)
#define H2C_STAGE 4
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_links_calls_msgs(const h2c_link* __restrict__ tab, uint32_t nlinks) {
  H2C_OF(blockIdx.x / H2C_LINK_GRID)
#define H2C_STAGE 5
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_links_calls_cols(const h2c_link* __restrict__ tab, uint32_t nlinks) {
  H2C_OF(blockIdx.x / H2C_LINK_GRID)
#define H2C_STAGE 6
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
// (one workgroup per link: H2C_BLK is not used by the stage, H2C_NBLK is the number of runs it sums)
__global__ __launch_bounds__(H2C_THREADS) void k_h2_links_calls_finish(const h2c_link* __restrict__ tab, uint32_t nlinks) {
  H2C_OF(blockIdx.x)
  uint64_t* const R = H2C_ENTRY(tab, blockIdx.x).res;
#define H2C_STAGE 7
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
__global__ __launch_bounds__(H2C_THREADS) void k_h2_links_calls_emit(const h2c_link* __restrict__ tab, uint32_t nlinks) {
  H2C_OF(blockIdx.x / H2C_LINK_GRID)
#define H2C_STAGE 8
#include "grdma_h2_calls_stage.inc"
#undef H2C_STAGE
}
#undef H2C_OF
#undef H2C_BLK
#undef H2C_NBLK

}  // namespace
#endif  // GRDMA_H2_CALLS_H
