// Header blocks, sending (grdma_h2_hpenc, "the header encoder"): header lists in the layout the header decoder writes -- a
// block table, a field table and a string arena in device memory -- encoded (HPACK, RFC 7541) against the PEER's dynamic
// table into the wire bytes of HEADERS and CONTINUATION frames, with no host step between a decode and the encode of its
// output.  The rules stand in include/grdma_amd.h ("Header blocks, sending"); the sequential reference is
// tests/h2_hpenc_model.py.  The encoder belongs to no parser: it is the sending side.
//
// A field of a block is an OCCURRENCE: occurrence i of the call is field first_field + (i - the occurrences in front of
// its block).  Four launches of fixed shape:
//   k_h2_hpenc_scan    a lane per field of the field table: the strings' bounds, their Huffman lengths (a 256-byte
//                      length table in LDS), the name hash and the full hash (FNV-1a), and the match against the 61
//                      static entries by hash, then by bytes: the lowest index whose name and value are equal, the
//                      lowest whose name is
//   k_h2_hpenc_walk    one workgroup: the peer's dynamic table as a ring of 2048 entries in LDS -- two hashes, two
//                      lengths, and where the strings ARE: the persistent byte ring, or this call's string arena for an
//                      entry this call inserted, so nothing waits for a copy.  The blocks' ranges and stream ids, a
//                      block scan of their field counts; then the occurrences in steps of 256, one a thread: every
//                      thread finds its block among the places of 257 blocks staged in LDS (behind them only after a
//                      run of empty blocks) and looks its field up against the table in front of the step (newest
//                      entry first, hashes nominate, bytes decide).  The first occurrence in wire order that must insert is taken by ONE
//                      thread -- evictions, the ring slot -- and the occurrences behind it are patched in O(1): an
//                      entry they had matched and that is gone leaves no older match either, and the new entry is one
//                      more candidate.  That repeats until no occurrence of the step inserts (after warm-up: at once).
//                      Then every occurrence's representation, index and size, a block scan for its place, a second
//                      pass over the blocks for their lengths, frame counts and places in the wire arena, the totals
//                      against the caps, the result block and, unless refused, the commit of ring and counters: the
//                      only stage that changes persistent state (the byte copies of k_h2_hpenc_commit aside, which it
//                      lists)
//   k_h2_hpenc_emit    a lane per occurrence writes its prefix integer and its strings, raw or Huffman-coded, through the
//                      position function (byte p of a block at base lies at base + 9 (p / max_frame + 1) + p: a field
//                      may be cut by a frame anywhere); a lane per block writes its frame headers, the size updates in
//                      front of the call's first block and the block-wire entry.  Nothing after a refusal.
//   k_h2_hpenc_commit  the strings of the entries this call inserted and that survive, from the string arena into the
//                      byte ring
// No global atomic: order comes from prefix sums and from the one thread of the walk.  Kernel boundaries are the only
// agent-scope hand-over.  The stages' bodies are source text (csrc/grdma_h2_hpenc_stage.inc), laid out as the header
// decoder's; the k_h2_links_hpenc_* kernels at the end of the file include the same text over a table of links.
#ifndef GRDMA_H2_HPENC_H
#define GRDMA_H2_HPENC_H
#include "grdma_h2_hpack.h"
#include "grdma_h2_hpenc_tables.h"

#define H2HE_THREADS 256
#ifdef GRDMA_WAVE_EMU
#define H2HE_GRID 2  // (the emulator runs workgroups one after another)
#else
#define H2HE_GRID 64
#endif
#define H2HE_CHUNK H2HE_THREADS  // occurrences per step of the walk: one a thread
#define H2HE_NONE 0xffffffffu

enum { H2HE_BLOCKS = 0, H2HE_FRAMES = 1, H2HE_WIRE = 2, H2HE_INSERTED = 3, H2HE_EVICTED = 4, H2HE_TABLE = 5, H2HE_FLAGS = 6,
       H2HE_OVERFLOW = 7 };
enum { H2HE_F_BAD_INPUT = 1 };  // GRDMA_H2_HPENC_BAD_INPUT of include/grdma_amd.h
enum { H2HE_E_FIELD_RANGE = 1, H2HE_E_STREAM = 2, H2HE_E_LENGTH = 3, H2HE_E_STRING = 4, H2HE_E_BLOCK_TOO_LARGE = 5 };
enum { H2HE_OVER_CAPS = 1, H2HE_OVER_SCRATCH = 3 };  // the overflow word: 3 never leaves the host call (it grows the table and repeats)

struct h2he_wire_out { uint64_t off; uint32_t len, nframes; };  // grdma_h2_header_wire
// a field as the scan leaves it: the hashes; the strings' encoded lengths | Huffman << 31; st = the lowest static index
// with the field's name and value | the lowest with its name << 8 | what is wrong with it (H2HE_E_*) << 16
struct h2he_rec { uint32_t hn, hf, nenc, venc, st, rsv[3]; };
// an occurrence as the walk resolves it: where its bytes begin among the call's block bytes; w = index (of the field, or
// of the name) | representation << 28; its block
struct h2he_occ { uint64_t pos; uint32_t w, blk; };
// a block: the occurrences in front of it; where its bytes begin among the call's block bytes; where its frames begin in
// the wire arena, their bytes and their number
struct h2he_blk { uint64_t occ0, pstart, woff; uint32_t len, nframes; };
struct h2he_job { uint32_t name_src, value_src, dst, name_len, value_len, rsv; };  // string arena offsets -> byte ring offset

// one call (the host's words)
struct h2he_call {
  const h2hp_block_out* blocks;
  uint64_t nblocks;
  const h2hp_field_out* fields;
  uint64_t nfields;
  const uint8_t* strings;
  uint64_t strings_bytes;
  uint8_t* wire;
  uint64_t wire_cap;
  h2he_wire_out* bw;
  uint64_t bw_cap;
  h2he_rec* recs;  // one per field
  uint64_t recs_cap;
  h2he_occ* occs;  // one per occurrence
  uint64_t occs_cap;
  h2he_blk* blks;  // one per block and one behind
  uint64_t blks_cap;
  uint32_t max_frame, nupd, upd[2];  // the size updates in front of the call's first block
};

// the encoder, resident in HBM
struct h2he_dev {
  h2he_call c;
  // state and counters since creation (the device's)
  uint32_t cur_max, size, cnt, ins;  // as h2hp_dev's: entry i lives at slot i % H2HP_RING
  uint32_t ring_head, pad0;
  uint64_t st_calls, st_blocks, st_fields, st_list, st_wire, st_inserted, st_evicted;
  // a call's scratch
  uint64_t res[8];  // H2HE_*
  uint64_t nocc;    // occurrences of the call (after H2HE_OVER_SCRATCH: how many the table must hold)
  uint32_t njobs, go;  // strings to copy into the byte ring; the call stands: emit and commit run
  h2he_job jobs[H2HP_RING];
  uint32_t r_hn[H2HP_RING], r_hf[H2HP_RING], r_nl[H2HP_RING], r_vl[H2HP_RING], r_src[H2HP_RING];  // the value stands behind the name
  uint8_t bytes[H2HP_BYTES];
  // tables (uploaded at create)
  uint32_t huff_code[256];
  uint8_t huff_bits[256];
  uint32_t st_hn[64], st_hf[64];
  uint16_t st_off[2 * 62 + 2];
  uint8_t st_bytes[H2HP_STATIC_BYTES];
};

namespace {

__device__ __forceinline__ uint32_t h2he_fnv(uint32_t h, uint32_t b) { return (h ^ b) * 0x01000193u; }
// bytes of a minimal integer under an nbits prefix
__device__ __forceinline__ uint32_t h2he_int_len(uint32_t v, uint32_t nbits) {
  const uint32_t limit = (1u << nbits) - 1u;
  if (v < limit) return 1u;
  uint32_t n = 2u;
  for (v -= limit; v >= 128u; v >>= 7) n++;
  return n;
}
// ... of a string whose encoded length | Huffman << 31 is e
__device__ __forceinline__ uint32_t h2he_str_len(uint32_t e) {
  const uint32_t n = e & 0x7fffffffu;
  return h2he_int_len(n, 7) + n;
}
// n bytes at s against the n at base from src on, which wrap under mask (the byte ring's; ~0 for a flat buffer).  To the
// end, with no way out at the first difference: the hashes and the lengths were equal, so the strings almost always are,
// and a loop that may leave waits for memory once a byte where this one has its loads in flight together.
__device__ __forceinline__ bool h2he_eq(const uint8_t* base, uint32_t src, uint32_t mask, const uint8_t* s, uint32_t n) {
  uint32_t diff = 0;
  for (uint32_t k = 0; k < n; k++) diff |= (uint32_t)(base[(src + k) & mask] ^ s[k]);
  return diff == 0;
}
// a table entry's string (fresh: in this call's string arena, else in the byte ring) against n bytes at s
__device__ __forceinline__ bool h2he_same(const h2he_dev* F, const h2he_call* C, bool fresh, uint32_t src, const uint8_t* s, uint32_t n) {
  return h2he_eq(fresh ? C->strings : F->bytes, src, fresh ? 0xffffffffu : H2HP_BYTES - 1u, s, n);
}

// where a block's bytes go: byte p of the block lies at base + 9 (p / max_frame + 1) + p
struct h2he_out {
  uint8_t* at;
  const uint8_t* end;  // of the block's frames
  uint32_t room, max_frame;
};
__device__ __forceinline__ h2he_out h2he_open(uint8_t* base, uint32_t len, uint64_t p, uint32_t max_frame) {
  const uint64_t q = p / max_frame;
  return {base + 9u * (q + 1u) + p, base + len, max_frame - (uint32_t)(p - q * max_frame), max_frame};
}
__device__ __forceinline__ void h2he_put(h2he_out& o, uint32_t b) {
  if (o.at < o.end) *o.at = (uint8_t)b;  // (cannot fail: the walk summed the same lengths)
  o.at++;
  if (--o.room == 0) {
    o.at += 9;
    o.room = o.max_frame;
  }
}
__device__ __forceinline__ void h2he_put_int(h2he_out& o, uint32_t v, uint32_t nbits, uint32_t first) {
  const uint32_t limit = (1u << nbits) - 1u;
  if (v < limit) {
    h2he_put(o, first | v);
    return;
  }
  h2he_put(o, first | limit);
  for (v -= limit; v >= 128u; v >>= 7) h2he_put(o, 0x80u | (v & 0x7fu));
  h2he_put(o, v);
}
// a string of n bytes at s, e its encoded length | Huffman << 31; code / bits: the Huffman code (in LDS)
__device__ __forceinline__ void h2he_put_str(h2he_out& o, const uint8_t* s, uint32_t n, uint32_t e, const uint32_t* code, const uint8_t* bits) {
  h2he_put_int(o, e & 0x7fffffffu, 7, (e >> 31) ? 0x80u : 0u);
  if (!(e >> 31)) {
    for (uint32_t k = 0; k < n; k++) h2he_put(o, s[k]);
    return;
  }
  uint64_t acc = 0;
  uint32_t have = 0;  // (at most 7 bits wait: 7 + 30 fit)
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t b = s[k], ln = bits[b];
    acc = (acc << ln) | code[b];
    have += ln;
    while (have >= 8u) {
      have -= 8u;
      h2he_put(o, (uint32_t)(acc >> have) & 0xffu);
    }
  }
  if (have) h2he_put(o, ((uint32_t)(acc << (8u - have)) & 0xffu) | (0xffu >> have));
}

#define H2HE_BLK blockIdx.x
#define H2HE_NBLK H2HE_GRID
#define H2HE_ONE                        \
  const h2he_call* const C = &F->c;     \
  uint64_t* const R = F->res;           \
  uint64_t* const N = &F->nocc;
__global__ __launch_bounds__(H2HE_THREADS) void k_h2_hpenc_scan(h2he_dev* F) {
  H2HE_ONE
#define H2HE_STAGE 1
#include "grdma_h2_hpenc_stage.inc"
#undef H2HE_STAGE
}
__global__ __launch_bounds__(H2HE_THREADS) void k_h2_hpenc_walk(h2he_dev* F) {
  H2HE_ONE
#define H2HE_STAGE 2
#include "grdma_h2_hpenc_stage.inc"
#undef H2HE_STAGE
}
__global__ __launch_bounds__(H2HE_THREADS) void k_h2_hpenc_emit(h2he_dev* F) {
  H2HE_ONE
#define H2HE_STAGE 3
#include "grdma_h2_hpenc_stage.inc"
#undef H2HE_STAGE
}
__global__ __launch_bounds__(H2HE_THREADS) void k_h2_hpenc_commit(h2he_dev* F) {
  H2HE_ONE
#define H2HE_STAGE 4
#include "grdma_h2_hpenc_stage.inc"
#undef H2HE_STAGE
}
#undef H2HE_ONE
#undef H2HE_BLK
#undef H2HE_NBLK

// ---- the four stages over a table of L <= H2HE_LINKS_MAX links: four launches however many links.  Nothing is shared
// between the links: every entry has its own h2he_dev (ring, counters, the hand-overs go, njobs and jobs between the
// launches), its own call words and its own nine result words, so bad input, a cap overflow, an occurrence table too
// small or a call without blocks stay with their link, and each link commits or refuses as its single call would.  The
// call words and the result words stand in the batch block of the host call (one copy up, one copy down for all links),
// not in the encoders' blocks.  The walk runs one workgroup per link (its 48 KiB of LDS let three links share a compute
// unit); in the grid stages link l owns the workgroups [l * H2HE_LINK_GRID, (l + 1) * H2HE_LINK_GRID).
#define H2HE_LINKS_MAX 256  // (= GRDMA_H2_BATCH_MAX, include/grdma_amd.h)
#ifdef GRDMA_WAVE_EMU
#define H2HE_LINK_GRID 2
#else
#define H2HE_LINK_GRID 4    // (256 links: 1024 workgroups, four to a compute unit)
#endif
struct h2he_link {
  h2he_dev* F;
  const h2he_call* call;  // in the batch block
  uint64_t* res;          // the item's nine words in the batch block: H2HE_*, then the occurrence count
};
// (the table is written by the host in front of the launch and only read on the device: constant memory, as H2HP_ENTRY)
#ifdef GRDMA_WAVE_EMU
#define H2HE_ENTRY(tab, l) ((tab)[l])
#else
#define H2HE_ENTRY(tab, l) (((const __attribute__((address_space(4))) h2he_link*)(tab))[l])
#endif

#define H2HE_BLK (blockIdx.x % H2HE_LINK_GRID)
#define H2HE_NBLK H2HE_LINK_GRID
#define H2HE_OF(l)                                       \
  if ((l) >= nlinks) return;                             \
  h2he_dev* const F = H2HE_ENTRY(tab, l).F;              \
  const h2he_call* const C = H2HE_ENTRY(tab, l).call;    \
  uint64_t* const R = H2HE_ENTRY(tab, l).res;            \
  uint64_t* const N = R + 8;
__global__ __launch_bounds__(H2HE_THREADS) void k_h2_links_hpenc_scan(const h2he_link* __restrict__ tab, uint32_t nlinks) {
  H2HE_OF(blockIdx.x / H2HE_LINK_GRID)
#define H2HE_STAGE 1
#include "grdma_h2_hpenc_stage.inc"
#undef H2HE_STAGE
}
__global__ __launch_bounds__(H2HE_THREADS) void k_h2_links_hpenc_walk(const h2he_link* __restrict__ tab, uint32_t nlinks) {
  H2HE_OF(blockIdx.x)
#define H2HE_STAGE 2
#include "grdma_h2_hpenc_stage.inc"
#undef H2HE_STAGE
}
__global__ __launch_bounds__(H2HE_THREADS) void k_h2_links_hpenc_emit(const h2he_link* __restrict__ tab, uint32_t nlinks) {
  H2HE_OF(blockIdx.x / H2HE_LINK_GRID)
#define H2HE_STAGE 3
#include "grdma_h2_hpenc_stage.inc"
#undef H2HE_STAGE
}
__global__ __launch_bounds__(H2HE_THREADS) void k_h2_links_hpenc_commit(const h2he_link* __restrict__ tab, uint32_t nlinks) {
  H2HE_OF(blockIdx.x / H2HE_LINK_GRID)
#define H2HE_STAGE 4
#include "grdma_h2_hpenc_stage.inc"
#undef H2HE_STAGE
}
#undef H2HE_OF
#undef H2HE_BLK
#undef H2HE_NBLK

}  // namespace
#endif  // GRDMA_H2_HPENC_H
