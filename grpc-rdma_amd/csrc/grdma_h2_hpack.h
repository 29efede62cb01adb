// Header blocks on the device (grdma_h2_hpack, "the header decoder"): the HPACK (RFC 7541) blocks of a deframing's
// HEADERS and CONTINUATION frames decoded into device memory -- a block table, a field table and a string arena -- with
// no host step in between, so that a server can route on :path and a client can read grpc-status where the bytes are.
// The rules stand in include/grdma_amd.h ("Header blocks"); the sequential reference is tests/h2_hpack_model.py.
//
// A frame's payload is the run of PAYLOAD events behind its FRAME event; the deframer lets nothing but CONTINUATION
// frames of the same stream follow a HEADERS frame without END_HEADERS, so blocks do not interleave, the order of their
// HEADERS frames is the order of their completions, and only the LAST block of a call can be open at its end.
//
// Seven launches of fixed shape behind a deframing (the event count is read on the device), in two host steps: the
// gather runs first and says how many fragment bytes the call holds, the host sizes the staging buffer and the record
// table by that figure (not by the call's bytes, which are mostly DATA) and launches the rest:
//   k_h2_hpack_gather  one workgroup, one thread per event in steps of 256: a FRAME thread walks the PAYLOAD events of
//                      its frame (bounded by the next FRAME event, the frame's end and the event count) -- how much of
//                      it is in, the pad length, whether it is complete; a block scan over fragment lengths and block
//                      starts gives every header frame its place in the staging buffer and every block its number.
//                      The carried frame and block are item 0 in front of the events.  Padding and size errors.
//   k_h2_hpack_copy    the carried fragment and every header frame's fragment bytes into the staging buffer: blocks are
//                      contiguous there
//   k_h2_hpack_split   one lane per block, the Huffman automaton in LDS: the field boundaries -- integer prefixes and
//                      string lengths, the decoded length of every Huffman string -- one record per field at the slot
//                      of the block's first byte + the field's number (a field has at least one byte)
//   k_h2_hpack_walk    one workgroup: the dynamic table as a ring of 2048 descriptors in LDS.  The records of as many
//                      blocks as fit are staged in LDS by all threads.  The records between two that change the table
//                      (an insertion, a size update) see one table: every thread resolves one, a block scan gives the
//                      offsets in the string arena; ONE thread takes the record that changes the table (evictions,
//                      the insertion).  All threads write the resolved fields out.  An entry's strings are named by where their bytes ARE -- the static table, a literal
//                      in the staging buffer, the persistent byte ring -- so no field waits for another field's bytes.
//                      Then the totals against the caps, the result block and, unless a cap overflowed, the commit of
//                      ring, counters and carry: the only stage that changes persistent state (the two byte copies of
//                      k_h2_hpack_commit aside, which it lists)
//   k_h2_hpack_emit    one lane per string: copies or Huffman-decodes it to its offset in the string arena; one thread
//                      per field and per block for the tables.  Nothing after an overflow.
//   k_h2_hpack_commit  the strings of the entries this call inserted and that survive, from the string arena into the
//                      byte ring; the open block's bytes into the carry buffer
// and k_h2_hpack_resize, one thread, for grdma_h2_hpack_set_max_table_size.
// No global atomic: order comes from prefix sums and from the one thread of the walk.  Kernel boundaries are the only
// agent-scope hand-over.  The stages' bodies are source text (csrc/grdma_h2_hpack_stage.inc), laid out as the control-
// reply writer's; the k_h2_links_hpack_* kernels at the end of the file include the same text over a table of links.
#ifndef GRDMA_H2_HPACK_H
#define GRDMA_H2_HPACK_H
#include "grdma_h2_kernels.h"
#include "grdma_h2_hpack_tables.h"

#define H2HP_THREADS 256
#ifdef GRDMA_WAVE_EMU
#define H2HP_GRID 2  // (the emulator runs workgroups one after another)
#else
#define H2HP_GRID 64
#endif
#define H2HP_RING 2048u        // live entries at most: 65536 / 32
#define H2HP_BYTES 65536u      // the byte ring: an entry's strings are fewer bytes than the table size
#define H2HP_CHUNK 512u        // field records staged per step of the walk
#define H2HP_MAX_TABLE 65536u
#define H2HP_NONE 0xffffffffu

enum { H2HP_BLOCKS = 0, H2HP_FIELDS = 1, H2HP_STRINGS = 2, H2HP_INSERTED = 3, H2HP_EVICTED = 4, H2HP_TABLE = 5, H2HP_FLAGS = 6,
       H2HP_OVERFLOW = 7 };
enum { H2HP_F_FAILED = 1, H2HP_F_LOST = 2, H2HP_F_OPEN = 4 };  // GRDMA_H2_HPACK_* of include/grdma_amd.h
enum { H2HP_E_PADDING = 1, H2HP_E_BLOCK_TOO_LARGE = 2, H2HP_E_INTEGER = 3, H2HP_E_TRUNCATED = 4, H2HP_E_HUFFMAN = 5, H2HP_E_INDEX = 6,
       H2HP_E_SIZE_UPDATE = 7, H2HP_E_DEFRAMER = 8 };
// where a string's bytes are: kind << 30 | position
enum { H2HP_S_STATIC = 0u,    // position: index | 256 for the value
       H2HP_S_STAGE = 1u,     // position of the string's length prefix in the staging buffer
       H2HP_S_RING = 2u };    // offset in the byte ring
#define H2HP_SRC(kind, pos) (((uint32_t)(kind) << 30) | (uint32_t)(pos))

struct h2hp_call {  // one call: where the deframer left its output and what it read (h2ctl_call's members)
  const grdma_h2_event* ev;
  const grdma_h2_deframe_result* res;
  const grdma_slice_out* sl;
  const uint8_t* arena;
  uint64_t ev_cap, nsl;
  uint64_t skipped;
};
struct h2hp_block_out { uint32_t stream, first_field, nfields, flags; };          // grdma_h2_header_block
struct h2hp_field_out { uint32_t name_off, value_off, name_len, value_len; };     // grdma_h2_header_field
// what a call's end leaves behind: the open frame (any type) and the open block
struct h2hp_carry {
  uint32_t type1, flags, size, seen;  // the open frame: its type + 1 (0: none), flags, size, payload bytes seen
  uint32_t pad;                      // its pad length, H2HP_NONE: not in (or not padded)
  uint32_t in_block;                 // a block is open
  uint32_t blk_stream, blk_flags;    // of its HEADERS frame, as the block table has them
  uint32_t frag_len, rsv[3];         // bytes in the carry buffer
};
struct h2hp_item { uint32_t dst, lo, hi, seen0; };  // a header frame: payload bytes [lo, hi) go to the staging buffer from dst on
// a block: where it stands in the staging buffer; records (fields and size updates), fields, fields in front of it
struct h2hp_blk { uint32_t off, len, stream, flags, err, nrec, nfields, first; };
// a field as the split leaves it: w0 = index | representation << 24 | size update << 28; positions of the strings'
// length prefixes in the staging buffer; decoded lengths; rsv its block.  As the walk resolves it: w0 = representation,
// name_pos / value_pos = where the strings are (H2HP_SRC), the lengths, the offsets in the string arena.
struct h2hp_rec { uint32_t w0, name_pos, value_pos, name_len, value_len, name_off, value_off, rsv; };
struct h2hp_entry { uint32_t name_src, name_len, value_src, value_len; };
struct h2hp_job { uint32_t src, dst, len, rsv; };  // string arena offset -> byte ring offset

// the decoder, resident in HBM
struct h2hp_dev {
  // where a call writes (the host sets it)
  h2hp_block_out* blocks;
  uint64_t blocks_cap;
  h2hp_field_out* fields;
  uint64_t fields_cap;
  uint8_t* strings;
  uint64_t strings_cap;
  // a call's scratch (the host's: sized between the two steps)
  uint8_t* stage;
  uint64_t stage_cap;
  h2hp_rec* recs;  // one slot per staging byte
  uint64_t recs_cap;
  h2hp_rec* outs;  // the resolved fields, in order
  uint64_t outs_cap;
  h2hp_item* items;  // one per event + 1
  h2hp_blk* blks;
  uint64_t items_cap;
  // configuration
  uint8_t* carry_buf;
  uint64_t max_block;
  uint32_t setting, pad0;
  // state and counters since creation (the device's)
  h2hp_carry carry, carry_out;
  uint32_t cur_max, size, cnt, ins;  // size limit, bytes, live entries, insertions so far (entry i lives at ring[i % H2HP_RING])
  uint32_t ring_head, pad1;          // where the byte ring grows
  uint64_t sticky;                   // flags | error << 8 | stream << 32
  uint64_t st_calls, st_blocks, st_fields, st_strings, st_inserted, st_evicted;
  // a call's scratch
  uint64_t pre[4];  // the gather's: fragment bytes with the carry, blocks (the open one included), the last block is open, -
  uint64_t res[8];  // H2HP_*
  uint32_t good_blocks, njobs;  // blocks delivered; strings to copy into the byte ring
  uint32_t open_off, open_len;  // the open block in the staging buffer
  h2hp_job jobs[H2HP_RING];
  h2hp_entry ring[H2HP_RING];
  uint8_t bytes[H2HP_BYTES];
  // tables (uploaded at create)
  uint32_t huff[H2HP_HUFF_WORDS];
  uint16_t st_off[2 * 62 + 2];  // name of entry i: st_bytes[st_off[2 i] .. st_off[2 i + 1]), value: .. st_off[2 i + 2])
  uint8_t st_bytes[H2HP_STATIC_BYTES];
};

namespace {

__device__ __forceinline__ bool h2hp_lost(const h2hp_call* call) { return call->res->overflow || call->res->nevents > call->ev_cap; }
__device__ __forceinline__ bool h2hp_is_header(uint32_t type) { return type == FT_HEADERS || type == FT_CONTINUATION; }
// bytes of a HEADERS frame's payload in front of the fragment
__device__ __forceinline__ uint32_t h2hp_lo(uint32_t type, uint32_t flags) {
  return type == FT_HEADERS ? ((flags & 0x8u) ? 1u : 0u) + ((flags & 0x20u) ? 5u : 0u) : 0u;
}
__device__ __forceinline__ const uint8_t* h2hp_piece(const h2hp_call* call, const grdma_h2_event& pe) {
  if (pe.slice >= call->nsl) return nullptr;
  const grdma_slice_out sl = call->sl[pe.slice];
  if ((uint64_t)pe.a + pe.b > sl.len) return nullptr;
  return call->arena + sl.off + pe.a;
}

// The payload of the frame whose PAYLOAD events begin at event j: how far it gets in this call (pos: in, payload bytes
// seen before; out, seen now), its pad length where it is wanted and in, whether it completes.  Bounded by the event
// count, the next frame and the frame's end.
__device__ __forceinline__ bool h2hp_walk_frame(const h2hp_call* call, uint64_t j, uint64_t n, bool padded, uint32_t& pos, uint32_t& pad) {
  for (; j < n; j++) {
    const grdma_h2_event e = call->ev[j];
    if (e.kind == EV_FRAME) {
      if (e.a != 0xffu) return false;  // (cannot be: a frame ends before the next begins)
      continue;
    }
    if (e.kind != EV_PAYLOAD) continue;
    if (padded && pad == H2HP_NONE && pos == 0 && e.b > 0) {
      const uint8_t* src = h2hp_piece(call, e);
      pad = src ? src[0] : 0u;
    }
    pos += e.b;
    if (e.c) return true;
  }
  return false;
}

// An HPACK integer with an nbits prefix at pos of blk[0, end): -> 0 or the error; at most five continuation bytes, at
// most 2^32 - 1.
__device__ __forceinline__ uint32_t h2hp_int(const uint8_t* blk, uint32_t& pos, uint32_t end, uint32_t nbits, uint32_t& out) {
  if (pos >= end) return H2HP_E_TRUNCATED;
  const uint32_t limit = (1u << nbits) - 1u;
  uint64_t v = blk[pos++] & limit;
  if (v == limit) {
    uint32_t k = 0;
    for (;; k++) {
      if (k == 5) return H2HP_E_INTEGER;
      if (pos >= end) return H2HP_E_TRUNCATED;
      const uint32_t b = blk[pos++];
      v += (uint64_t)(b & 0x7fu) << (7 * k);
      if (!(b & 0x80u)) break;
    }
    if (v > 0xffffffffull) return H2HP_E_INTEGER;
  }
  out = (uint32_t)v;
  return 0;
}

// The Huffman string src[0, n) through the automaton A (in LDS): its decoded length, or H2HP_NONE for EOS inside it or a
// padding that is none.  dst: where the bytes go, cap of them at most (NULL: the length only).
__device__ __forceinline__ uint32_t h2hp_huffman(const uint32_t* A, const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t cap) {
  uint32_t st = 0, len = 0, accept = H2HP_HUFF_ACCEPT;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t b = src[i];
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const uint32_t e = A[st * 16u + (half ? (b & 15u) : (b >> 4))];
      if (e & H2HP_HUFF_FAIL) return H2HP_NONE;
      if (e & H2HP_HUFF_EMIT) {
        if (dst && len < cap) dst[len] = (uint8_t)(e >> 16);
        len++;
      }
      st = e & 0xffu;
      accept = e & H2HP_HUFF_ACCEPT;
    }
  }
  return accept ? len : H2HP_NONE;
}

// A string (length prefix at pos) of blk[0, end): steps over it; its decoded length.  -> 0 or the error
__device__ __forceinline__ uint32_t h2hp_string(const uint32_t* A, const uint8_t* blk, uint32_t& pos, uint32_t end, uint32_t& len) {
  if (pos >= end) return H2HP_E_TRUNCATED;
  const uint32_t h = blk[pos] & 0x80u;
  uint32_t n = 0;
  if (const uint32_t err = h2hp_int(blk, pos, end, 7, n)) return err;
  if (n > end - pos) return H2HP_E_TRUNCATED;
  len = n;
  if (h) {
    len = h2hp_huffman(A, blk + pos, n, nullptr, 0);
    if (len == H2HP_NONE) return H2HP_E_HUFFMAN;
  }
  pos += n;
  return 0;
}

// A field against the table as it stands (cnt live entries, ins insertions so far): where its name and its value are and
// how long.  false: an index that is none.
__device__ __forceinline__ bool h2hp_resolve(const h2hp_rec& r, const h2hp_entry* ring, const uint16_t* stlen, uint32_t cnt, uint32_t ins,
                                             uint32_t& nsrc, uint32_t& nlen, uint32_t& vsrc, uint32_t& vlen) {
  const uint32_t idx = r.w0 & 0xffffffu, rep = (r.w0 >> 24) & 3u;
  if (idx) {
    if (idx < 62u) {
      nsrc = H2HP_SRC(H2HP_S_STATIC, idx);
      nlen = stlen[2u * idx];
      vsrc = H2HP_SRC(H2HP_S_STATIC, idx | 256u);
      vlen = stlen[2u * idx + 1u];
    } else if (idx - 62u < cnt) {
      const h2hp_entry e = ring[(ins - 1u - (idx - 62u)) & (H2HP_RING - 1u)];
      nsrc = e.name_src;
      nlen = e.name_len;
      vsrc = e.value_src;
      vlen = e.value_len;
    } else {
      return false;
    }
  } else if (rep == 0) {
    return false;
  } else {
    nsrc = H2HP_SRC(H2HP_S_STAGE, r.name_pos);
    nlen = r.name_len;
  }
  if (rep) {
    vsrc = H2HP_SRC(H2HP_S_STAGE, r.value_pos);
    vlen = r.value_len;
  }
  return true;
}

// the oldest entries go until `need` more bytes fit under limit (thread 0 of the walk, and the resize)
#define H2HP_EVICT(ring, need, limit)                                          \
  while (cnt && (uint64_t)size + (need) > (limit)) {                           \
    const h2hp_entry old = (ring)[(ins - cnt) & (H2HP_RING - 1u)];             \
    size -= 32u + old.name_len + old.value_len;                                \
    cnt--;                                                                     \
    evicted++;                                                                 \
  }

#define H2HP_BLK blockIdx.x
#define H2HP_NBLK H2HP_GRID
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_hpack_gather(h2hp_dev* F, const h2hp_call* call) {
#define H2HP_STAGE 1
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_hpack_copy(h2hp_dev* F, const h2hp_call* call) {
#define H2HP_STAGE 2
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_hpack_split(h2hp_dev* F, const h2hp_call* call) {
#define H2HP_STAGE 3
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_hpack_walk(h2hp_dev* F, const h2hp_call* call) {
#define H2HP_STAGE 4
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_hpack_emit(h2hp_dev* F, const h2hp_call* call) {
#define H2HP_STAGE 5
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_hpack_commit(h2hp_dev* F, const h2hp_call* call) {
#define H2HP_STAGE 6
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(64) void k_h2_hpack_resize(h2hp_dev* F) {
#define H2HP_STAGE 7
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
#undef H2HP_BLK
#undef H2HP_NBLK

// ---- the six stages over a table of L <= H2HP_LINKS_MAX links: six launches however many links.  Nothing is shared
// between the links: every entry has its own h2hp_dev (targets, scratch, carry, ring, counters, result block) and its own
// call block, so a sticky error, a lost call, a deframer error, a cap overflow or an empty event list stay with their
// link, and each link commits or refuses as its single call would.  The gather and the walk run one workgroup per link
// (the walk's LDS lets two links share a compute unit); in the grid stages link l owns the workgroups
// [l * H2HP_LINK_GRID, (l + 1) * H2HP_LINK_GRID).  There is no resize over links.
#define H2HP_LINKS_MAX 256  // (= GRDMA_H2_BATCH_MAX, include/grdma_amd.h)
#ifdef GRDMA_WAVE_EMU
#define H2HP_LINK_GRID 2
#else
#define H2HP_LINK_GRID 4    // (256 links: 1024 workgroups, four to a compute unit)
#endif
struct h2hp_link {
  h2hp_dev* F;
  const h2hp_call* call;
};
// (the table is written by the host in front of the launch and only read on the device: constant memory, as H2CTL_ENTRY)
#ifdef GRDMA_WAVE_EMU
#define H2HP_ENTRY(tab, l) ((tab)[l])
#else
#define H2HP_ENTRY(tab, l) (((const __attribute__((address_space(4))) h2hp_link*)(tab))[l])
#endif

#define H2HP_BLK (blockIdx.x % H2HP_LINK_GRID)
#define H2HP_NBLK H2HP_LINK_GRID
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_links_hpack_gather(const h2hp_link* __restrict__ tab, uint32_t nlinks) {
  if (blockIdx.x >= nlinks) return;
  h2hp_dev* const F = H2HP_ENTRY(tab, blockIdx.x).F;
  const h2hp_call* const call = H2HP_ENTRY(tab, blockIdx.x).call;
#define H2HP_STAGE 1
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_links_hpack_copy(const h2hp_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2HP_LINK_GRID;
  if (l >= nlinks) return;
  h2hp_dev* const F = H2HP_ENTRY(tab, l).F;
  const h2hp_call* const call = H2HP_ENTRY(tab, l).call;
#define H2HP_STAGE 2
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_links_hpack_split(const h2hp_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2HP_LINK_GRID;
  if (l >= nlinks) return;
  h2hp_dev* const F = H2HP_ENTRY(tab, l).F;
  const h2hp_call* const call = H2HP_ENTRY(tab, l).call;
#define H2HP_STAGE 3
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_links_hpack_walk(const h2hp_link* __restrict__ tab, uint32_t nlinks) {
  if (blockIdx.x >= nlinks) return;
  h2hp_dev* const F = H2HP_ENTRY(tab, blockIdx.x).F;
  const h2hp_call* const call = H2HP_ENTRY(tab, blockIdx.x).call;
#define H2HP_STAGE 4
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_links_hpack_emit(const h2hp_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2HP_LINK_GRID;
  if (l >= nlinks) return;
  h2hp_dev* const F = H2HP_ENTRY(tab, l).F;
  const h2hp_call* const call = H2HP_ENTRY(tab, l).call;
#define H2HP_STAGE 5
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
__global__ __launch_bounds__(H2HP_THREADS) void k_h2_links_hpack_commit(const h2hp_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2HP_LINK_GRID;
  if (l >= nlinks) return;
  h2hp_dev* const F = H2HP_ENTRY(tab, l).F;
  const h2hp_call* const call = H2HP_ENTRY(tab, l).call;
#define H2HP_STAGE 6
#include "grdma_h2_hpack_stage.inc"
#undef H2HP_STAGE
}
#undef H2HP_BLK
#undef H2HP_NBLK

}  // namespace
#endif  // GRDMA_H2_HPACK_H
