// The message assembler (grdma_h2_asm): the deframer's events -> gRPC messages, contiguous in a ring over a device
// arena the caller provides, plus one 32-byte descriptor per message (grdma_h2_rx_msg).  The consumer side of the
// receive path: chttp2's incoming byte stream feeding the surface's receive_message (call.cc receiving_slice_ready /
// continue_receiving_slices append slices to the call's grpc_byte_buffer), with the length check of the message_size
// filter (message_size_filter.cc: RESOURCE_EXHAUSTED "Received message larger than max").
//
// Six kernels in one linear chain behind the deframer; none returns to the host, and every launch shape is fixed (the
// event count is read from the deframe result on the device).  The keyed state of an event is
//   S = (kind: none / open message begun at event idx / no message, bytes since),   combine(a, b) = b.kind ? b : a + b.bytes
// over the earlier events of the same stream (MSG_BEGIN = (open, i, 0), MSG_BYTES = (none, -, len), MSG_END and
// STREAM_CLOSED = (no message, -, 0)).  kind none means "what the stream carried into the call" (the assembler's own
// per-stream table).
//   k_h2_asm_tiles    wave tiles of 64 events: per distinct stream of the tile (ballot + readfirstlane, a masked scan)
//                     the tile's aggregate; per tile the count and granule bytes of its MSG_BEGINs
//   k_h2_asm_carry    one workgroup: tile prefixes (block scans), the allocation plan as four scalars (where the ring
//                     wraps, where the call runs out of space or records), and the keyed scan over the tile aggregates
//                     (one wave, 64 aggregates per step, running state per stream in an LDS hash)
//   k_h2_asm_begin    per MSG_BEGIN: status, offset, seq, record
//   k_h2_asm_bytes    per MSG_BYTES: its message and fill -> a copy piece {src, dst, len}; per MSG_END / STREAM_CLOSED
//                     that finishes a message: its descriptor (in event order, placed by the next kernel)
//   k_h2_asm_finish   one workgroup: descriptor positions (block scan), the carried table, truncation on a connection
//                     error
//   k_h2_asm_copy     fixed grid: descriptors to their places; the pieces cut into 4 KiB copy tiles (a prefix sum of
//                     each piece's tile count), taken by static grid-stride and moved with wave_copy_tile_g
// k_h2_asm_release (one wave) releases reported messages in reported order and moves the ring's tail.
// The stages' bodies are source text (csrc/grdma_h2_asm_stage.inc); the k_h2_asm_*_links kernels at the end of this file
// run the same six stages (and the release) over a table of links: six launches however many transports.
#ifndef GRDMA_H2_ASM_H
#define GRDMA_H2_ASM_H
#include "grdma_h2_kernels.h"

#define H2A_THREADS 256
#define H2A_ONE_THREADS 512
#ifdef GRDMA_WAVE_EMU
#define H2A_GRID 2  // (the emulator runs workgroups one after another: the kernels are grid-stride)
#else
#define H2A_GRID 512
#endif
#define H2A_GRANULE 256ull
#define H2A_COPY_TILE 4096ull  // what wave_copy_tile_g moves with all its loads in flight (4 x 16 B per lane)
static_assert(H2A_COPY_TILE == GRDMA_COPY_G_BYTES, "a copy tile of the assembler is what wave_copy_tile_g holds in registers");
#define H2A_LDS_KEYS 4096u   // distinct streams with message events in one call, at most 3/4 of this
#define H2A_NONE 0u
#define H2A_OPEN 1u
#define H2A_SHUT 2u

// one keyed element / state
struct h2a_el {
  uint32_t kind, idx;
  uint64_t bytes;
};
// a stream's aggregate over one wave tile (k_h2_asm_tiles), then its exclusive prefix over the call (k_h2_asm_carry)
struct h2a_key {
  uint32_t key, kind, idx, pad;
  uint64_t bytes, pad2;
};
struct h2a_tile {
  uint32_t nkeys, nbeg, nrep, ncopy;   // ncopy: the copy tiles of the wave tile's pieces
  uint64_t bsz;                        // granule bytes of the tile's MSG_BEGINs (too large ones: 0)
  uint64_t key_base, beg_base, sz_base, rep_base, copy_base;
};
// what a MSG_BEGIN decided (k_h2_asm_begin), per event
struct h2a_msg {
  uint64_t offset, length, seq, rec;   // rec = ~0: no record (NO_SPACE)
  uint32_t stream, status, flags, pad;
};
// a message a stream carries from one call into the next (open addressing, linear probing from (id >> 1) & mask,
// backward-shift deletion: the parser's stream map scheme)
struct h2a_carry {
  uint32_t stream_id, status, flags, pad;
  uint64_t offset, length, seq, rec, fill;
};
// one allocation record (a ring of max_pending); rank = report rank, ~0 until reported
struct h2a_rec {
  uint64_t vstart, vend, rank, freed;
};
struct h2a_piece {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t len;
  uint64_t tpre;                       // copy tiles of the wave tile's earlier pieces
};
// one call: where the deframer left its output (standalone calls and every pipe have their own)
struct h2a_call {
  const grdma_h2_event* ev;
  const grdma_h2_deframe_result* res;
  const grdma_slice_out* sl;
  const uint8_t* src_arena;
  uint64_t ev_cap;
  uint64_t release_all;                // a pipe step first releases everything reported before it
};
// the assembler, resident in HBM
struct h2a_dev {
  uint8_t* arena;
  uint64_t arena_bytes, max_msg, max_pending;
  uint32_t tab_mask, pad0;
  h2a_carry* tab;
  h2a_rec* recs;
  // scratch of one call (capacity scratch_ev events)
  uint64_t scratch_ev;
  h2a_tile* tiles;
  h2a_key* keys;
  uint32_t* comp;
  h2a_key* fin;
  h2a_msg* msgs;
  h2a_piece* pieces;
  grdma_h2_rx_msg* dtmp;               // per event: the descriptor it reports (pad = 1)
  grdma_h2_rx_msg* desc;               // the call's descriptors
  uint64_t desc_cap;
  // ring and counters
  uint64_t vh, vt;                     // virtual head / tail (physical = v % arena_bytes)
  uint64_t rec_head, rec_tail;
  uint64_t seq, reported, released;
  // the plan of the current call (k_h2_asm_carry)
  uint64_t n, skip, nfin;
  uint64_t wrap_ord, c_wrap, waste, cutoff, seq_base, rec_base, vh0;
  uint64_t ndesc, rank_base, ncopy;    // ncopy: copy tiles of the call
  // counters since creation: reported, OK bytes, too large, no space, truncated
  uint64_t st_reported, st_ok_bytes, st_too_large, st_no_space, st_trunc;
};

namespace {

__device__ __forceinline__ h2a_el h2a_combine(h2a_el a, h2a_el b) {
  if (b.kind) return b;
  a.bytes += b.bytes;
  return a;
}

// inclusive scan of combine over the 64 lanes (non-members hold the identity {0, 0, 0})
__device__ __forceinline__ h2a_el h2a_wave_scan(h2a_el v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    h2a_el o;
    o.kind = __shfl_up(v.kind, d, 64);
    o.idx = __shfl_up(v.idx, d, 64);
    o.bytes = __shfl_up(v.bytes, d, 64);
    if (lane >= d) v = h2a_combine(o, v);
  }
  return v;
}

__device__ __forceinline__ uint64_t h2a_gran(uint64_t len) { return (len + H2A_GRANULE - 1) & ~(H2A_GRANULE - 1); }

// the keyed element of one event (key 0 = none)
__device__ __forceinline__ void h2a_elem_of(const grdma_h2_event& e, uint32_t* key, h2a_el* el, uint32_t i) {
  *key = 0;
  *el = h2a_el{0, 0, 0};
  if (e.kind == 3) {
    *key = e.c;
    *el = h2a_el{H2A_OPEN, i, 0};
  } else if (e.kind == 4) {
    *key = e.c;
    el->bytes = e.b;
  } else if (e.kind == 5 || e.kind == 7) {
    *key = e.c;
    el->kind = H2A_SHUT;
  }
}

// size in the ring of the MSG_BEGIN e (0: zero length or too large)
__device__ __forceinline__ uint64_t h2a_size_of(const h2a_dev* A, const grdma_h2_event& e) {
  if (e.kind != 3) return 0;
  if (A->max_msg && e.b > A->max_msg) return 0;
  return h2a_gran(e.b);
}

__device__ __forceinline__ uint64_t h2a_tab_find(const h2a_dev* A, uint32_t id) {
  uint32_t s = (id >> 1) & A->tab_mask;
  for (uint32_t probe = 0; probe <= A->tab_mask; probe++, s = (s + 1) & A->tab_mask) {
    const uint32_t k = A->tab[s].stream_id;
    if (k == id) return s;
    if (k == 0) return ~0ull;
  }
  return ~0ull;
}

__device__ __forceinline__ void h2a_tab_delete(h2a_dev* A, uint64_t slot) {
  const uint32_t m = A->tab_mask;
  uint32_t i = (uint32_t)slot;
  A->tab[i].stream_id = 0;
  uint32_t j = i;
  for (;;) {
    j = (j + 1) & m;
    const uint32_t k = A->tab[j].stream_id;
    if (k == 0) return;
    const uint32_t home = (k >> 1) & m;
    // move j back into the hole i unless its home lies cyclically in (i, j]
    const bool stays = (i <= j) ? (home > i && home <= j) : (home > i || home <= j);
    if (!stays) {
      A->tab[i] = A->tab[j];
      A->tab[j].stream_id = 0;
      i = j;
    }
  }
}

__device__ __forceinline__ void h2a_tab_put(h2a_dev* A, const h2a_carry& c) {
  uint32_t s = (c.stream_id >> 1) & A->tab_mask;
  for (uint32_t probe = 0; probe <= A->tab_mask; probe++, s = (s + 1) & A->tab_mask) {
    const uint32_t k = A->tab[s].stream_id;
    if (k == c.stream_id || k == 0) {
      A->tab[s] = c;
      return;
    }
  }
}

// release: everything reported (all) or `count` more, then the tail over released / freed records.  One wave.
__device__ void h2a_release_wave(h2a_dev* A, uint64_t count, bool all, int lane) {
  uint64_t rel = A->released;
  rel = all ? A->reported : (count > A->reported - rel ? A->reported : rel + count);
  uint64_t t = A->rec_tail;
  const uint64_t h = A->rec_head;
  const uint64_t P = A->max_pending;
  while (t < h) {
    const uint64_t r = t + (uint64_t)lane;
    bool live = false;
    if (r < h) {
      const h2a_rec& rc = A->recs[r % P];
      live = !(rc.freed || rc.rank < rel);
    }
    const uint64_t in = r < h ? 1 : 0;
    const uint64_t lm = __ballot(live && in);
    if (lm) {
      t += (uint64_t)__builtin_ctzll(lm);
      break;
    }
    t += 64;
    if (t > h) t = h;
  }
  uint64_t vt = A->vh;
  if (t < h) vt = A->recs[t % P].vstart;
  if (lane == 0) {
    A->released = rel;
    A->rec_tail = t;
    A->vt = vt;
  }
}

__global__ __launch_bounds__(64) void k_h2_asm_release(h2a_dev* A, uint64_t count) {
  h2a_release_wave(A, count, false, (int)threadIdx.x);
}

// The stages' bodies are source text (csrc/grdma_h2_asm_stage.inc) shared with the many-link kernels at the end of this
// file; for the single-transport kernels the grid is the call's.
#define H2A_BLK blockIdx.x
#define H2A_NBLK gridDim.x
// ---- 1. per wave tile: the aggregate of every stream in it, the tile's MSG_BEGINs
__global__ __launch_bounds__(H2A_THREADS) void k_h2_asm_tiles(h2a_dev* A, const h2a_call* call) {
#define H2A_STAGE 1
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
}

// block-wide exclusive scan of v over H2A_ONE_THREADS threads (ws: 16 words of LDS); *total = the sum
__device__ __forceinline__ uint64_t h2a_block_scan(uint64_t v, uint64_t* ws, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t incl = wave_incl_scan(v, lane);
  if (lane == 63) ws[wave] = incl;
  __syncthreads();
  uint64_t base = 0, tot = 0;
  for (int w = 0; w < H2A_ONE_THREADS / 64; w++) {
    const uint64_t s = ws[w];
    if (w < wave) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

// the first begin ordinal in tile t (or ~0) whose "key" crosses the bound: crosses(C exclusive, size) per MSG_BEGIN
template <typename F>
__device__ __forceinline__ uint64_t h2a_first_in_tile(const h2a_dev* A, const h2a_call* call, uint64_t t, uint64_t n,
                                                      F crosses, uint64_t* c_at, int lane) {
  const uint64_t i = t * 64 + lane;
  grdma_h2_event e{0, 0, 0, 0, 0, 0};
  if (i < n) e = call->ev[i];
  const uint64_t sz = h2a_size_of(A, e);
  const uint64_t c = A->tiles[t].sz_base + wave_incl_scan(sz, lane) - sz;
  const bool beg = e.kind == 3 && i < n;
  const uint64_t bm = __ballot(beg);
  const uint64_t ord = A->tiles[t].beg_base + (uint64_t)__builtin_popcountll(bm & ((1ull << lane) - 1));
  const uint64_t hit = __ballot(beg && crosses(c, sz));
  if (!hit) return ~0ull;
  const int f = __builtin_ctzll(hit);
  *c_at = (uint64_t)__shfl(c, f, 64);
  return (uint64_t)__shfl(ord, f, 64);
}

// ---- 2. one workgroup: tile prefixes, the allocation plan, the keyed scan over the tile aggregates
__global__ __launch_bounds__(H2A_ONE_THREADS) void k_h2_asm_carry(h2a_dev* A, const h2a_call* call) {
#define H2A_STAGE 2
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
}

// the start (virtual) of MSG_BEGIN ordinal k with exclusive size prefix c and size s
__device__ __forceinline__ uint64_t h2a_start(const h2a_dev* A, uint64_t k, uint64_t c) {
  const bool wrapped = A->wrap_ord != ~0ull && k >= A->wrap_ord;
  return wrapped ? A->vh0 + A->waste + c : A->vh0 + c;
}

// ---- 3. per MSG_BEGIN: status, offset, seq, record
__global__ __launch_bounds__(H2A_THREADS) void k_h2_asm_begin(h2a_dev* A, const h2a_call* call) {
#define H2A_STAGE 3
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
}

// ---- 4. per MSG_BYTES: its message and fill (a copy piece); per finishing event: its descriptor
__global__ __launch_bounds__(H2A_THREADS) void k_h2_asm_bytes(h2a_dev* A, const h2a_call* call) {
#define H2A_STAGE 4
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
}

// ---- 5. one workgroup: descriptor positions, the carried table, truncation on a connection error
__global__ __launch_bounds__(H2A_ONE_THREADS) void k_h2_asm_finish(h2a_dev* A, const h2a_call* call) {
#define H2A_STAGE 5
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
}

// ---- 6. descriptors to their places; then the copy tiles of all pieces (4 KiB each, GRDMA prefix of k_h2_asm_finish) by
// static grid-stride: wave w moves tiles w, w + W, w + 2 W, ...  Its 64 lanes first find the pieces of 64 of its tiles at
// once (binary searches over the wave tiles' copy_base, then over the pieces' tpre), then the wave moves them one by one.
__device__ __forceinline__ uint64_t h2a_last_le_tile(const h2a_dev* A, uint64_t ntiles, uint64_t c) {
  uint64_t lo = 0, hi = ntiles;  // the last wave tile whose copy_base <= c (a tile without pieces shares its base with the next)
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) / 2;
    if (A->tiles[mid].copy_base <= c) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(H2A_THREADS) void k_h2_asm_copy(h2a_dev* A, const h2a_call* call) {
  (void)call;
  if (A->skip) return;
  const uint64_t n = A->n;
  const int lane = threadIdx.x & 63;
  const uint64_t ntiles = (n + 63) / 64;
  const uint64_t waves = (uint64_t)gridDim.x * (H2A_THREADS / 64);
  const uint64_t wave = blockIdx.x * (H2A_THREADS / 64) + (threadIdx.x >> 6);
  uint64_t ok_bytes = 0, too_large = 0, no_space = 0, trunc = 0;
#define H2A_STAGE 6
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
  const uint64_t T = A->ncopy;
  for (uint64_t k0 = 0; wave + k0 * waves < T; k0 += 64) {
    const uint64_t c = wave + (k0 + (uint64_t)lane) * waves;
    const uint8_t* src = nullptr;
    uint8_t* dst = nullptr;
    uint64_t len = 0;
    if (c < T) {
#define H2A_STAGE 7
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
    }
    uint64_t pm = __ballot(len != 0);
    while (pm) {
      const int p = __builtin_ctzll(pm);
      pm &= pm - 1;
      const uint8_t* s_ = (const uint8_t*)uni64((uint64_t)__shfl((uint64_t)src, p, 64));
      uint8_t* d_ = (uint8_t*)uni64((uint64_t)__shfl((uint64_t)dst, p, 64));
      const uint64_t m = uni64(__shfl(len, p, 64));
      wave_copy_tile_g(d_, s_, m, lane);
    }
  }
  // (counters: one atomic per lane that counted something)
  if (ok_bytes) atomicAdd((unsigned long long*)&A->st_ok_bytes, (unsigned long long)ok_bytes);
  if (too_large) atomicAdd((unsigned long long*)&A->st_too_large, (unsigned long long)too_large);
  if (no_space) atomicAdd((unsigned long long*)&A->st_no_space, (unsigned long long)no_space);
  if (trunc) atomicAdd((unsigned long long*)&A->st_trunc, (unsigned long long)trunc);
}
#undef H2A_BLK
#undef H2A_NBLK

// ---- the six stages over a table of L <= H2A_LINKS_MAX links (transports of a batch, links of a group pipe): six
// launches per step however many links.  Nothing is shared between the links -- every entry has its own assembler block,
// scratch, ring and call block -- so an event overflow, too many streams, NO_SPACE or a connection error stay with
// their link.  The entry is loaded with a uniform index: it sits in scalar registers, as the single-transport kernels'
// parameters do (k_h2_deframe_links does the same).
//   tiles, begin, bytes   link l owns the workgroups [l * H2A_LINK_GRID, (l + 1) * H2A_LINK_GRID): the single kernel's
//                         grid-stride over wave tiles inside that share
//   carry, finish         grid L: workgroup l is the one workgroup of link l -- L plans side by side
//   copy                  descriptors per link (shares of H2A_LINK_GRID workgroups, dealt over the grid); the copy tiles
//                         of ALL links by one static grid-stride, so an idle link idles nobody: every workgroup builds
//                         the exclusive prefix of the links' tile counts in LDS (one block scan), a lane finds the link
//                         of its tile by binary search over it and then the piece inside the link as k_h2_asm_copy does
// The kernel boundary is the only agent-scope hand-over; inside a workgroup barriers only.
#define H2A_LINKS_MAX 256  // (= GRDMA_H2_BATCH_MAX, include/grdma_amd.h; one thread per link in the copy's block scan)
#ifdef GRDMA_WAVE_EMU
#define H2A_LINK_GRID H2A_GRID
#else
#define H2A_LINK_GRID 8    // 32 waves per link: a wave per wave tile up to 2048 events, grid-stride beyond
#endif
struct h2a_link {
  h2a_dev* A;
  const h2a_call* call;
};
struct h2a_link_release {
  h2a_dev* A;
  uint64_t count;
};
static_assert(H2A_LINKS_MAX <= H2A_THREADS, "k_h2_asm_copy_links scans one link per thread");

__global__ __launch_bounds__(64) void k_h2_asm_release_links(const h2a_link_release* __restrict__ tab) {
  const h2a_link_release e = tab[blockIdx.x];
  h2a_release_wave(e.A, e.count, false, (int)threadIdx.x);
}

// (a link's share of the grid)
#define H2A_BLK (blockIdx.x % H2A_LINK_GRID)
#define H2A_NBLK H2A_LINK_GRID
__global__ __launch_bounds__(H2A_THREADS) void k_h2_asm_tiles_links(const h2a_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2A_LINK_GRID;
  if (l >= nlinks) return;
  const h2a_link e = tab[l];
  h2a_dev* const A = e.A;
  const h2a_call* const call = e.call;
#define H2A_STAGE 1
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
}

__global__ __launch_bounds__(H2A_ONE_THREADS) void k_h2_asm_carry_links(const h2a_link* __restrict__ tab) {
  const h2a_link e = tab[blockIdx.x];
  h2a_dev* const A = e.A;
  const h2a_call* const call = e.call;
#define H2A_STAGE 2
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
}

__global__ __launch_bounds__(H2A_THREADS) void k_h2_asm_begin_links(const h2a_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2A_LINK_GRID;
  if (l >= nlinks) return;
  const h2a_link e = tab[l];
  h2a_dev* const A = e.A;
  const h2a_call* const call = e.call;
#define H2A_STAGE 3
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
}

__global__ __launch_bounds__(H2A_THREADS) void k_h2_asm_bytes_links(const h2a_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2A_LINK_GRID;
  if (l >= nlinks) return;
  const h2a_link e = tab[l];
  h2a_dev* const A = e.A;
  const h2a_call* const call = e.call;
#define H2A_STAGE 4
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
}
#undef H2A_BLK
#undef H2A_NBLK

__global__ __launch_bounds__(H2A_ONE_THREADS) void k_h2_asm_finish_links(const h2a_link* __restrict__ tab) {
  const h2a_link e = tab[blockIdx.x];
  h2a_dev* const A = e.A;
  const h2a_call* const call = e.call;
#define H2A_STAGE 5
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
}

__global__ __launch_bounds__(H2A_THREADS) void k_h2_asm_copy_links(const h2a_link* __restrict__ tab, uint32_t nlinks) {
  __shared__ uint64_t s_pre[H2A_LINKS_MAX + 1];  // exclusive prefix of the links' copy tiles; [nlinks ..]: the total
  __shared__ uint64_t s_wave[H2A_THREADS / 64];
  const int lane = threadIdx.x & 63;
  const uint32_t wv = threadIdx.x >> 6;
  // descriptors to their places: share v % H2A_LINK_GRID of link v / H2A_LINK_GRID, the shares dealt over the grid
  for (uint32_t v = blockIdx.x; v < nlinks * H2A_LINK_GRID; v += gridDim.x) {
    const h2a_link e = tab[v / H2A_LINK_GRID];
    h2a_dev* const A = e.A;
    if (A->skip) continue;
    const uint64_t n = A->n;
    const uint64_t ntiles = (n + 63) / 64;
    const uint64_t waves = (uint64_t)H2A_LINK_GRID * (H2A_THREADS / 64);
    const uint64_t wave = (v % H2A_LINK_GRID) * (H2A_THREADS / 64) + wv;
    uint64_t ok_bytes = 0, too_large = 0, no_space = 0, trunc = 0;
#define H2A_STAGE 6
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
    if (ok_bytes) atomicAdd((unsigned long long*)&A->st_ok_bytes, (unsigned long long)ok_bytes);
    if (too_large) atomicAdd((unsigned long long*)&A->st_too_large, (unsigned long long)too_large);
    if (no_space) atomicAdd((unsigned long long*)&A->st_no_space, (unsigned long long)no_space);
    if (trunc) atomicAdd((unsigned long long*)&A->st_trunc, (unsigned long long)trunc);
  }
  // the links' copy tiles in front of each link (a link whose call failed has none)
  uint64_t mine = 0;
  if (threadIdx.x < nlinks) {
    const h2a_dev* const A = tab[threadIdx.x].A;
    if (!A->skip) mine = A->ncopy;
  }
  const uint64_t incl = wave_incl_scan(mine, lane);
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  uint64_t base = 0;
  for (uint32_t w = 0; w < wv; w++) base += s_wave[w];
  if (threadIdx.x == 0) s_pre[0] = 0;
  s_pre[threadIdx.x + 1] = base + incl;
  __syncthreads();
  const uint64_t T = s_pre[nlinks];
  const uint64_t waves = (uint64_t)gridDim.x * (H2A_THREADS / 64);
  const uint64_t wave = blockIdx.x * (H2A_THREADS / 64) + wv;
  for (uint64_t k0 = 0; wave + k0 * waves < T; k0 += 64) {
    const uint64_t g = wave + (k0 + (uint64_t)lane) * waves;
    const uint8_t* src = nullptr;
    uint8_t* dst = nullptr;
    uint64_t len = 0;
    if (g < T) {
      uint32_t ll = 0, lh = nlinks;  // the last link whose prefix <= g (a link without tiles shares its prefix with the next)
      while (lh - ll > 1) {
        const uint32_t mid = (ll + lh) / 2;
        if (s_pre[mid] <= g) ll = mid;
        else lh = mid;
      }
      const h2a_dev* const A = tab[ll].A;
      const uint64_t n = A->n;
      const uint64_t ntiles = (n + 63) / 64;
      const uint64_t c = g - s_pre[ll];
#define H2A_STAGE 7
#include "grdma_h2_asm_stage.inc"
#undef H2A_STAGE
    }
    uint64_t pm = __ballot(len != 0);
    while (pm) {
      const int p = __builtin_ctzll(pm);
      pm &= pm - 1;
      const uint8_t* s_ = (const uint8_t*)uni64((uint64_t)__shfl((uint64_t)src, p, 64));
      uint8_t* d_ = (uint8_t*)uni64((uint64_t)__shfl((uint64_t)dst, p, 64));
      const uint64_t m = uni64(__shfl(len, p, 64));
      wave_copy_tile_g(d_, s_, m, lane);
    }
  }
}


}  // namespace
#endif  // GRDMA_H2_ASM_H
