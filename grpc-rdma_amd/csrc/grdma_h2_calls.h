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
// Kernel boundaries are the only agent-scope hand-over.
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

// the run of n items workgroup w takes: [*b0, *b1), a multiple of the workgroup's threads long
__device__ __forceinline__ void h2c_run(uint64_t n, uint32_t w, uint64_t* b0, uint64_t* b1) {
  uint64_t per = (n + H2C_GRID - 1u) / H2C_GRID;
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

__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_clear(h2c_dev* F) {
  const h2c_call* const C = &F->c;
  const uint64_t tid = (uint64_t)blockIdx.x * H2C_THREADS + threadIdx.x, nth = (uint64_t)H2C_GRID * H2C_THREADS;
  h2c_entry* const neu = F->tab[1u - F->cur];
  const uint32_t slots = F->slots;
  const h2c_entry e0 = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const h2c_aux a0 = {H2C_NONE, H2C_NONE, 0, 0, 0, 0, 0, 0};
  for (uint64_t s = tid; s < slots; s += nth) neu[s] = e0, F->aux[s] = a0;
  for (uint64_t s = tid; s <= C->dd_mask; s += nth) C->dd[s] = h2c_dd{0, H2C_NONE};
  for (uint64_t s = tid; s < (uint64_t)H2C_GRID * slots; s += nth) F->row_s[s] = 0;
  const uint32_t nk = F->nmethods + 1u;
  for (uint64_t s = tid; s < (uint64_t)H2C_GRID * H2C_KEYS_MAX; s += nth)
    if (s % H2C_KEYS_MAX < nk) F->row_k[s] = 0;
  if (tid < H2C_GRID) F->wins[tid] = 0, F->closes[tid] = 0, F->wg_bytes[tid] = 0;
  if (tid == 0) F->bad = ~0ull, F->nexp = 0, F->nleft = 0, F->go = 0;
}

__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_claim(h2c_dev* F) {
  const h2c_call* const C = &F->c;
  const uint64_t tid = (uint64_t)blockIdx.x * H2C_THREADS + threadIdx.x, nth = (uint64_t)H2C_GRID * H2C_THREADS;
  const h2c_entry* const old = F->tab[F->cur];
  const uint32_t mask = F->slots - 1u, nm = F->nmethods;
  for (uint64_t k = tid; k < C->nblocks; k += nth) {
    const uint32_t stream = C->meta[k].stream, word = C->meta[k].word, method = C->meta[k].method;
    uint32_t cls = H2C_CLS_NO;
    if (h2c_would_open(word, C->blocks[k].flags)) {
      const uint32_t code = (stream == 0 || (stream >> 31)) ? H2C_E_STREAM : method >= nm ? H2C_E_METHOD : 0u;
      if (code) {
        atomicMin(&F->bad, (unsigned long long)k << 8 | code);
      } else {
        const uint32_t s = h2c_find(old, mask, stream);
        if (s == H2C_NONE || (old[s].fin & H2C_EF_DEAD)) {  // (else a duplicate)
          const uint32_t d = h2c_claim(&C->dd[0].key, sizeof(h2c_dd) / 4u, (uint32_t)C->dd_mask, stream);
          if (d != H2C_NONE) {
            atomicMin(&C->dd[d].rec, (uint32_t)k);
            cls = H2C_CLS_CAND;
          }
        }
      }
    }
    C->cls[k] = cls;
  }
}

__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_wins(h2c_dev* F) {
  const h2c_call* const C = &F->c;
  const uint32_t tid = threadIdx.x;
  __shared__ uint32_t s_n[H2C_THREADS / 64];
  uint64_t b0, b1;
  h2c_run(C->nblocks, blockIdx.x, &b0, &b1);
  uint32_t n = 0;
  for (uint64_t k0 = b0; k0 < b1; k0 += H2C_THREADS) {  // (uniform)
    const uint64_t k = k0 + tid;
    bool win = false;
    if (k < b1 && C->cls[k] == H2C_CLS_CAND) {
      const uint32_t stream = C->meta[k].stream;
      uint32_t d = (stream >> 1) & (uint32_t)C->dd_mask;
      while (C->dd[d].key != stream) d = (d + 1u) & (uint32_t)C->dd_mask;  // (claimed in the stage before: it is there)
      win = C->dd[d].rec == (uint32_t)k;
      if (win) C->cls[k] = H2C_CLS_WIN;
    }
    n += (uint32_t)__builtin_popcountll(__ballot(win));
  }
  if ((tid & 63u) == 0) s_n[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
    for (uint32_t k = 0; k < H2C_THREADS / 64; k++) t += s_n[k];
    F->wins[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_insert(h2c_dev* F) {
  const h2c_call* const C = &F->c;
  const uint32_t tid = threadIdx.x;
  __shared__ uint64_t s_wave[H2C_THREADS / 64];
  static_assert(H2C_THREADS == PLAN_THREADS, "block_excl_scan is for this workgroup size");
  const h2c_entry* const old = F->tab[F->cur];
  h2c_entry* const neu = F->tab[1u - F->cur];
  const uint64_t now = C->now;
  // the live entries of the table behind the last step
  for (uint64_t s = (uint64_t)blockIdx.x * H2C_THREADS + tid; s < F->slots; s += (uint64_t)H2C_GRID * H2C_THREADS) {
    h2c_entry e = old[s];
    e.word |= e.fin;
    if (e.stream != 0 && !(e.fin & H2C_EF_DEAD)) h2c_put(F, neu, e, now);
  }
  // the winners of this run, in record order
  uint64_t run = 0;
  for (uint32_t w = 0; w < blockIdx.x; w++) run += F->wins[w];
  const uint64_t room = F->slots / 2u - F->live;  // (live <= slots / 2)
  uint64_t b0, b1;
  h2c_run(C->nblocks, blockIdx.x, &b0, &b1);
  for (uint64_t k0 = b0; k0 < b1; k0 += H2C_THREADS) {  // (uniform: the scan's barriers)
    const uint64_t k = k0 + tid;
    const bool win = k < b1 && C->cls[k] == H2C_CLS_WIN;
    uint64_t tot;
    const uint64_t rank = run + block_excl_scan(win ? 1ull : 0ull, s_wave, &tot);
    if (win && rank < room) {
      const h2m_meta_out r = C->meta[k];
      const uint64_t timeout = (uint64_t)r.timeout_lo | (uint64_t)r.timeout_hi << 32;
      uint64_t deadline = ~0ull;
      if ((r.word >> 24) & H2M_HAS_TIMEOUT) deadline = now + timeout < now ? ~0ull : now + timeout;
      const h2c_entry e = {F->serial + rank, deadline, 0, r.stream, r.method, 0, (r.word >> 16) & 0xffu, 0, 0};
      h2c_put(F, neu, e, now);
    }
    run += tot;
  }
}

__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_msgs(h2c_dev* F) {
  const h2c_call* const C = &F->c;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  h2c_entry* const neu = F->tab[1u - F->cur];
  const uint32_t mask = F->slots - 1u, nm = F->nmethods;
  uint32_t* const row_s = F->row_s + (size_t)blockIdx.x * F->slots;
  uint32_t* const row_k = F->row_k + (size_t)blockIdx.x * H2C_KEYS_MAX;
  // the closing events: the lowest LEFT and the lowest reads-closed event of an entry
  for (uint64_t j = (uint64_t)blockIdx.x * H2C_THREADS + tid; j < C->nev; j += (uint64_t)H2C_GRID * H2C_THREADS) {
    const grdma_h2_event e = C->ev[j];
    if (e.kind != EV_STREAM_CLOSED || e.a > 1u || e.c == 0) continue;
    const uint32_t s = h2c_find(neu, mask, e.c);
    if (s != H2C_NONE) atomicMin(e.a ? &F->aux[s].left_at : &F->aux[s].rc_at, (uint32_t)j);
  }
  // the descriptors of this run, in order
  uint64_t b0, b1, bytes = 0;
  h2c_run(C->nmsgs, blockIdx.x, &b0, &b1);
  for (uint64_t i0 = b0; i0 < b1; i0 += H2C_THREADS) {  // (uniform)
    const uint64_t i = i0 + tid;
    const bool valid = i < b1;
    uint32_t slot = H2C_NONE, key = nm, reason = 0;
    uint64_t len = 0;
    if (valid) {
      const h2c_msg m = C->msgs[i];
      len = m.length;
      if (m.status != 0) {
        reason = H2C_BAD_STATUS;
      } else {
        const uint32_t s = m.stream ? h2c_find(neu, mask, m.stream) : H2C_NONE;
        if (s == H2C_NONE) {
          reason = H2C_NO_CALL;
        } else {
          const uint32_t word = neu[s].word;
          slot = s;
          if (word & H2C_EF_EXPIRED) reason = H2C_EXPIRED_MSG;
          else if ((m.flags & 1u) && (word & 0xffu) == 0) reason = H2C_COMPRESSED_IDENTITY;
          else key = neu[s].method;
        }
      }
    }
    const bool disp = valid && reason == 0;
    uint32_t rank_s, tot_s, rank_k, tot_k;
    bool last_s, last_k;
    h2c_keyed(slot, disp, lane, &rank_s, &tot_s, &last_s);
    h2c_keyed(key, valid, lane, &rank_k, &tot_k, &last_k);
    // the waves take turns at the run's rows: what the waves in front of this one added is in the row
    for (uint32_t v = 0; v < H2C_THREADS / 64; v++) {  // (uniform)
      if (wave == v) {
        if (disp) {
          const uint32_t base = row_s[slot];
          rank_s += base;
          if (last_s) row_s[slot] = base + tot_s;
        }
        if (valid) {
          const uint32_t base = row_k[key];
          rank_k += base;
          if (last_k) row_k[key] = base + tot_k;
        }
      }
      __syncthreads();
    }
    if (disp) {
      atomicAdd((unsigned long long*)&neu[slot].bytes, (unsigned long long)len);
      atomicAdd(&F->aux[slot].nstep, 1u);
      atomicMax(&F->aux[slot].last, (uint32_t)i + 1u);
      bytes += len;
    }
    if (valid) C->mrec[i] = h2c_mrec{slot, key, disp ? rank_s : reason, rank_k};
  }
  // the run's dispatched bytes (a sum: its order is free)
  for (int d = 32; d >= 1; d >>= 1) bytes += __shfl_xor(bytes, d, 64);
  if (lane == 0 && bytes) atomicAdd((unsigned long long*)&F->wg_bytes[blockIdx.x], (unsigned long long)bytes);
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

__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_cols(h2c_dev* F) {
  const h2c_call* const C = &F->c;
  const uint32_t tid = threadIdx.x;
  const uint64_t gid = (uint64_t)blockIdx.x * H2C_THREADS + tid, nth = (uint64_t)H2C_GRID * H2C_THREADS;
  const h2c_entry* const neu = F->tab[1u - F->cur];
  const uint32_t slots = F->slots, nk = F->nmethods + 1u;
  __shared__ uint32_t s_n[H2C_THREADS / 64];
  // down the rows: a key's, a slot's count in the runs in front
  for (uint64_t k = gid; k < nk; k += nth) {
    uint32_t acc = 0;
    for (uint32_t w = 0; w < H2C_GRID; w++) {
      const uint32_t t = F->row_k[(size_t)w * H2C_KEYS_MAX + k];
      F->row_k[(size_t)w * H2C_KEYS_MAX + k] = acc;
      acc += t;
    }
    F->ktot[k] = acc;
  }
  uint32_t nleft = 0;
  for (uint64_t s = gid; s < slots; s += nth) {
    if (neu[s].stream == 0) continue;
    uint32_t acc = 0;
    for (uint32_t w = 0; w < H2C_GRID; w++) {
      const uint32_t t = F->row_s[(size_t)w * slots + s];
      F->row_s[(size_t)w * slots + s] = acc;
      acc += t;
    }
    nleft += F->aux[s].left_at != H2C_NONE;
  }
  if (nleft) atomicAdd(&F->nleft, nleft);  // (a count: its order is free)
  // the newly expired: the rank by stream
  const uint32_t nexp = F->nexp < slots / 2u ? F->nexp : slots / 2u;
  for (uint64_t k = gid; k < nexp; k += nth) {
    const uint32_t mine = neu[F->exp_slot[k]].stream;
    uint32_t r = 0;
    for (uint32_t j = 0; j < nexp; j++) r += neu[F->exp_slot[j]].stream < mine;
    F->exp_rank[k] = r;
  }
  // the closes of this run of events
  uint64_t b0, b1;
  h2c_run(C->nev, blockIdx.x, &b0, &b1);
  uint32_t n = 0;
  for (uint64_t j0 = b0; j0 < b1; j0 += H2C_THREADS) {  // (uniform)
    const uint64_t j = j0 + tid;
    uint32_t slot;
    const bool mine = j < b1 && h2c_closes(F, neu, C->ev[j], j, &slot);
    n += (uint32_t)__builtin_popcountll(__ballot(mine));
  }
  if ((tid & 63u) == 0) s_n[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
    for (uint32_t k = 0; k < H2C_THREADS / 64; k++) t += s_n[k];
    F->closes[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_finish(h2c_dev* F) {
  const h2c_call* const C = &F->c;
  const uint32_t tid = threadIdx.x;
  __shared__ uint64_t s_wave[H2C_THREADS / 64];
  const uint32_t nm = F->nmethods, nk = nm + 1u;
  uint64_t* const R = F->res;
  const unsigned long long bad = F->bad;
  if (bad != ~0ull) {  // (uniform) the result block alone
    if (tid == 0) {
      for (int k = 0; k < 8; k++) R[k] = 0;
      R[H2C_FLAGS] = H2C_F_BAD_INPUT | (bad & 0xffu) << 8 | (bad >> 8) << 32;
    }
    return;
  }
  // the segments: the scan over the keys' totals (in place: ktot[k] becomes the start of k's segment, ktot[nk] the total)
  uint64_t run = 0;
  for (uint32_t k0 = 0; k0 < nk; k0 += H2C_THREADS) {  // (uniform: the scan's barriers)
    const uint32_t k = k0 + tid;
    const uint32_t v = k < nk ? F->ktot[k] : 0u;
    uint64_t tot;
    const uint64_t x = run + block_excl_scan((uint64_t)v, s_wave, &tot);
    if (k < nk) F->ktot[k] = (uint32_t)x;
    run += tot;
  }
  __syncthreads();
  if (tid != 0) return;
  F->ktot[nk] = (uint32_t)run;  // (= nmsgs)
  const uint64_t orphans = run - F->ktot[nm], dispatched = F->ktot[nm];
  uint64_t wins = 0, closes = 0, bytes = 0;
  for (uint32_t w = 0; w < H2C_GRID; w++) wins += F->wins[w], closes += F->closes[w], bytes += F->wg_bytes[w];
  const uint64_t room = F->slots / 2u - F->live, opened = wins < room ? wins : room;
  const uint32_t lost = F->lost | (wins > room ? 1u : 0u);
  const uint64_t nexp = F->nexp, ndone = nexp + closes, live = F->live + opened - F->nleft;
  const bool over = C->disp_cap < C->nmsgs || C->done_cap < ndone;
  R[H2C_OPENED] = opened;
  R[H2C_DISPATCHED] = dispatched;
  R[H2C_ORPHANS] = orphans;
  R[H2C_DONE] = ndone;
  R[H2C_EXPIRED] = nexp;
  R[H2C_LIVE] = live;
  R[H2C_FLAGS] = lost ? H2C_F_LOST : 0u;
  R[H2C_OVERFLOW] = over ? 1u : 0u;
  if (over) return;
  // the commit
  F->go = 1;
  F->emit_tab = 1u - F->cur;
  F->cur = 1u - F->cur;
  F->live = (uint32_t)live;
  F->lost = lost;
  F->serial += opened;
  F->st_steps += 1;
  F->st_opened += opened;
  F->st_msgs += dispatched;
  F->st_bytes += bytes;
  F->st_orphans += orphans;
  F->st_done += ndone;
}

__global__ __launch_bounds__(H2C_THREADS) void k_h2_calls_emit(h2c_dev* F) {
  if (!F->go) return;  // (uniform) bad input or a cap too small: nothing is written
  const h2c_call* const C = &F->c;
  const uint32_t tid = threadIdx.x;
  const uint64_t gid = (uint64_t)blockIdx.x * H2C_THREADS + tid, nth = (uint64_t)H2C_GRID * H2C_THREADS;
  __shared__ uint64_t s_wave[H2C_THREADS / 64];
  h2c_entry* const neu = F->tab[F->emit_tab];
  const uint32_t slots = F->slots, nm = F->nmethods;
  const uint32_t* const row_s = F->row_s + (size_t)blockIdx.x * slots;
  const uint32_t* const row_k = F->row_k + (size_t)blockIdx.x * H2C_KEYS_MAX;
  // the segment words, whole
  for (uint64_t k = gid; k < (uint64_t)nm + 2u; k += nth) C->segs[k] = F->ktot[k];
  // the dispatch records of this run
  uint64_t b0, b1;
  h2c_run(C->nmsgs, blockIdx.x, &b0, &b1);
  for (uint64_t i = b0 + tid; i < b1; i += H2C_THREADS) {
    const h2c_msg m = C->msgs[i];
    const h2c_mrec r = C->mrec[i];
    const uint64_t at = (uint64_t)F->ktot[r.key] + row_k[r.key] + r.rank_k;
    h2c_disp o = {m.offset, m.length, 0, m.stream, (uint32_t)i, H2C_NONE, (m.flags & 1u) ? (uint32_t)H2C_COMPRESSED : 0u, 0, 0};
    if (r.key != nm) {
      const h2c_aux a = F->aux[r.slot];
      o.call = neu[r.slot].call;
      o.method = r.key;
      o.seq = a.m0 + row_s[r.slot] + r.rank_s;
      o.word |= (neu[r.slot].word & 0xffu) << 16;
      if (o.seq == 0) o.word |= H2C_FIRST;
      if (a.last == (uint32_t)i + 1u && (a.left_at & a.rc_at) != H2C_NONE) o.word |= H2C_LAST;
    } else {
      o.word |= r.rank_s << 8;
      if (r.slot != H2C_NONE) o.call = neu[r.slot].call, o.word |= (neu[r.slot].word & 0xffu) << 16;
    }
    if (at < C->disp_cap) C->disp[at] = o;  // (at < nmsgs <= disp_cap)
  }
  // the done list: the deadlines by stream ...
  const uint32_t nexp = F->nexp < slots / 2u ? F->nexp : slots / 2u;
  for (uint64_t k = gid; k < nexp; k += nth) {
    const uint32_t s = F->exp_slot[k];
    const h2c_entry e = neu[s];
    // (an expired entry is dispatched nothing: its count and bytes are those it came with)
    const h2c_done o = {e.call, e.bytes, e.stream, e.method, e.messages, H2C_DEADLINE | ((e.word & H2C_EF_READS_CLOSED) ? 1u << 8 : 0u)};
    if (F->exp_rank[k] < C->done_cap) C->done[F->exp_rank[k]] = o;
  }
  // ... then the closes of this run of events, in event order
  uint64_t run = nexp;
  for (uint32_t w = 0; w < blockIdx.x; w++) run += F->closes[w];
  h2c_run(C->nev, blockIdx.x, &b0, &b1);
  for (uint64_t j0 = b0; j0 < b1; j0 += H2C_THREADS) {  // (uniform: the scan's barriers)
    const uint64_t j = j0 + tid;
    uint32_t s = 0;
    grdma_h2_event ev = {0, 0, 0, 0, 0, 0};
    if (j < b1) ev = C->ev[j];
    const bool mine = j < b1 && h2c_closes(F, neu, ev, j, &s);
    uint64_t tot;
    const uint64_t x = run + block_excl_scan(mine ? 1ull : 0ull, s_wave, &tot);
    if (mine && x < C->done_cap) {
      const h2c_aux a = F->aux[s];
      uint32_t word = H2C_READS_CLOSED;
      if (ev.a) word = H2C_LEFT | (((neu[s].word & H2C_EF_READS_CLOSED) || a.rc_at < a.left_at) ? 1u << 8 : 0u);
      const h2c_done o = {neu[s].call, neu[s].bytes, neu[s].stream, neu[s].method, a.m0 + a.nstep, word};
      C->done[x] = o;
    }
    run += tot;
  }
  // the entries made final: what the step's closes add goes into `fin`, which no stage of this step reads, and the count
  // of an entry another workgroup may still read (a DEADLINE record's) is an expired entry's, which does not change
  for (uint64_t s = gid; s < slots; s += nth) {
    if (neu[s].stream == 0) continue;
    const h2c_aux a = F->aux[s];
    neu[s].messages = a.m0 + a.nstep;
    neu[s].fin = (a.rc_at != H2C_NONE ? (uint32_t)H2C_EF_READS_CLOSED : 0u) | (a.left_at != H2C_NONE ? (uint32_t)H2C_EF_DEAD : 0u);
  }
}

}  // namespace
#endif  // GRDMA_H2_CALLS_H
