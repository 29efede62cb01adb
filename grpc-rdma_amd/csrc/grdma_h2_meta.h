// Call metadata (grdma_h2_meta, "the metadata reader"): the tables the header decoder writes -- a block table, a field
// table and a string arena in device memory -- read into one fixed-size call record per block (kind, verdict, method id,
// timeout, encoding, statuses, the field indices a later stage wants) and a compact list of rejection blocks over the
// reader's constant tables, which the header encoder turns into Trailers-Only responses with no host step in between.
// The rules stand in include/grdma_amd.h ("Call metadata"); the sequential reference is tests/h2_meta_model.py.  The
// reader belongs to no parser and keeps nothing between calls but its counters.
//
// Three launches of fixed shape:
//   k_h2_meta_fields  a lane per field of the field table: the strings' bounds; name and value walked four bytes an
//                     iteration (four loads in flight); the name's first 20 bytes, packed, against the known keys packed
//                     in LDS (equal lengths, then words); the legality of name and value; the value the key calls for
//                     from its first 17 bytes, packed (a timeout in nanoseconds, a status number, an encoding, POST,
//                     http(s), application/grpc, trailers) and for :path the probe of the method table (FNV-1a, hashed
//                     in the value's pass, nominates; bytes decide) -> a 16-byte record
//   k_h2_meta_blocks  a wave per block, a workgroup (sixteen waves) a contiguous run of blocks: the block's records in
//                     steps of 64, a ballot per known key -- the lowest lane of the first step that has it is the occurrence that
//                     counts -- and per lane the faults that need the fields in front of it (a pseudo-header twice,
//                     behind a regular field, :status beside a request pseudo-header) from the step's ballots and what
//                     the steps before left.  The wave writes the call record into scratch; the workgroup its counts
//   k_h2_meta_emit    every workgroup sums the counts in front of its run and the totals (a lane per count, shuffles);
//                     bad input or a cap too small end the call with the result block alone; else the records are copied out, the rejection blocks
//                     compacted in input order (a block scan per 256 blocks) and workgroup 0 writes the result block and
//                     bumps the counters
// No global atomic; kernel boundaries are the only agent-scope hand-over.  The stages' bodies are source text
// (csrc/grdma_h2_meta_stage.inc), laid out as the header encoder's; the k_h2_links_meta_* kernels at the end of the file
// include the same text over a table of links: three launches however many links, through the ONE reader.
#ifndef GRDMA_H2_META_H
#define GRDMA_H2_META_H
#include "grdma_h2_hpenc.h"
#include "grdma_h2_meta_tables.h"

#define H2M_THREADS 256
#define H2M_BLK_THREADS 1024  // of k_h2_meta_blocks: sixteen waves, so that a workgroup's run of 16 blocks is one block a wave
#ifdef GRDMA_WAVE_EMU
#define H2M_GRID 2  // (the emulator runs workgroups one after another)
#else
#define H2M_GRID 64
#endif
#define H2M_WG_BLOCKS 8u  // a workgroup takes this many blocks, or its share of the call's where that is more
#define H2M_NONE 0xffffffffu

enum { H2M_BLOCKS = 0, H2M_REQUESTS = 1, H2M_RESPONSES = 2, H2M_TRAILERS = 3, H2M_REJECTIONS = 4, H2M_MALFORMED = 5, H2M_FLAGS = 6,
       H2M_OVERFLOW = 7 };
enum { H2M_F_BAD_INPUT = 1 };  // GRDMA_H2_META_BAD_INPUT of include/grdma_amd.h
enum { H2M_E_FIELD_RANGE = 1, H2M_E_STREAM = 2, H2M_E_STRING = 3 };
enum { H2M_REQUEST = 1, H2M_RESPONSE = 2, H2M_IS_TRAILERS = 3 };
enum { H2M_OK = 0, H2M_V_MALFORMED, H2M_BAD_METHOD, H2M_BAD_CONTENT_TYPE, H2M_BAD_TE, H2M_BAD_TIMEOUT, H2M_UNIMPLEMENTED, H2M_BAD_ENCODING,
       H2M_HTTP_STATUS, H2M_NO_STATUS, H2M_BAD_GRPC_STATUS };
enum { H2M_HAS_TIMEOUT = 1, H2M_END_STREAM = 2, H2M_HAS_GRPC_STATUS = 4, H2M_HAS_MESSAGE = 8 };
// key ids (csrc/grdma_h2_meta_tables.h: position + 1)
enum { H2M_K_METHOD = 1, H2M_K_SCHEME, H2M_K_PATH, H2M_K_AUTHORITY, H2M_K_STATUS, H2M_K_CONTENT_TYPE, H2M_K_TE, H2M_K_TIMEOUT, H2M_K_ENCODING,
       H2M_K_ACCEPT, H2M_K_GRPC_STATUS, H2M_K_MESSAGE, H2M_K_LAST = H2M_K_MESSAGE };
// a field record's first word: the key | ...
enum { H2M_R_BAD = 1u << 8,      // a bad field (rule 2)
       H2M_R_GOOD = 1u << 9,     // the value is what the key calls for
       H2M_R_PSEUDO = 1u << 10,  // the name begins with ':'
       H2M_R_INPUT = 1u << 11 }; // a string leaves the arena

struct h2m_meta_out { uint32_t stream, word, method, http_status, grpc_status, timeout_lo, timeout_hi, path_field, authority_field,
                      message_field, ncustom, bad_field; };  // grdma_h2_call_meta
struct h2m_rec { uint32_t w, lo, hi, rsv; };           // a field as k_h2_meta_fields leaves it: H2M_R_*, the value's number
struct h2m_slot { uint32_t hash, off, len, id; };      // of the method table: len 0 is empty; the path's bytes at off
// what a workgroup of k_h2_meta_blocks counted in its run; bad: its first block with bad input << 8 | the code
struct h2m_wg { uint32_t rej, req, resp, trail, malformed, pad; uint64_t bad; };

// one call (the host's words)
struct h2m_call {
  const h2hp_block_out* blocks;
  uint64_t nblocks;
  const h2hp_field_out* fields;
  uint64_t nfields;
  const uint8_t* strings;
  uint64_t strings_bytes;
  h2m_meta_out* meta;
  uint64_t meta_cap;
  h2hp_block_out* reject;
  uint64_t reject_cap;
  h2m_rec* recs;       // one per field
  uint64_t recs_cap;
  h2m_meta_out* mrecs; // one per block
  uint64_t mrecs_cap;
};

// the reader, resident in HBM
struct h2m_dev {
  h2m_call c;
  uint64_t st_calls, st_blocks, st_requests, st_responses, st_trailers, st_rejections, st_malformed;  // since creation
  uint64_t res[8];  // H2M_*
  h2m_wg wg[H2M_GRID];
  // tables (uploaded at create)
  const h2m_slot* slots;
  const uint8_t* paths;
  uint32_t slot_mask, accept;
  uint32_t rej_first[16], rej_n[16];  // by verdict: the list in the constant field table
  uint8_t key_off[32];
  uint8_t key_bytes[256];
};

namespace {

// the run of blocks workgroup w of the nblk that share the blocks takes: [*b0, *b1)
__device__ __forceinline__ void h2m_run(uint64_t nblocks, uint32_t w, uint32_t nblk, uint64_t* b0, uint64_t* b1) {
  uint64_t per = (nblocks + nblk - 1u) / nblk;
  if (per < H2M_WG_BLOCKS) per = H2M_WG_BLOCKS;
  const uint64_t lo = per * w, hi = lo + per;
  *b0 = lo < nblocks ? lo : nblocks;
  *b1 = hi < nblocks ? hi : nblocks;
}
// a value's first bytes as the fields stage packs them (byte k at bits 8 k)
// (32-bit words: a comparison carries its literal, where a 64-bit one would hold a register pair across the loop)
#define H2M_LIT4(a, b, c, d) ((uint32_t)(uint8_t)(a) | (uint32_t)(uint8_t)(b) << 8 | (uint32_t)(uint8_t)(c) << 16 | (uint32_t)(uint8_t)(d) << 24)
#define H2M_IS8(a, b, c, d, e, f, g, h) (w0 == H2M_LIT4(a, b, c, d) && w1 == H2M_LIT4(e, f, g, h))
// the n <= 8 packed bytes of v as digits -> their number; false: not all digits
__device__ __forceinline__ bool h2m_number(uint64_t v, uint32_t n, uint32_t* out) {
  uint32_t x = 0, bad = 0;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t d = ((uint32_t)(v >> (8u * k)) & 0xffu) - 0x30u;
    bad |= d > 9u;
    x = x * 10u + d;
  }
  *out = x;
  return !bad;
}
// whether a verdict of a REQUEST gets a rejection block (rule 8)
__device__ __forceinline__ bool h2m_rejected(uint32_t word) {
  const uint32_t verdict = (word >> 8) & 0xffu;
  return (word & 0xffu) == H2M_REQUEST && verdict != H2M_OK && verdict != H2M_V_MALFORMED;
}
// lane src's v (src is the same in every lane)
__device__ __forceinline__ uint32_t h2m_from(uint32_t v, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane((int)src));
}

// the bytes [k, k + 4) of the n at s, byte j at bits 8 j, 0 behind the string's end (k < n): four loads in flight together,
// where a loop over bytes waits for memory once a byte
__device__ __forceinline__ uint32_t h2m_load4(const uint8_t* s, uint32_t k, uint32_t n) {
  uint32_t w = s[k];
  if (k + 1u < n) w |= (uint32_t)s[k + 1u] << 8;
  if (k + 2u < n) w |= (uint32_t)s[k + 2u] << 16;
  if (k + 3u < n) w |= (uint32_t)s[k + 3u] << 24;
  return w;
}

#define H2M_KEY_WORDS 5u  // a known key is at most 20 bytes
#define H2M_LINKS 0
#define H2M_BLK blockIdx.x
#define H2M_NBLK H2M_GRID
__global__ __launch_bounds__(H2M_THREADS) void k_h2_meta_fields(h2m_dev* F) {
  const h2m_call* const C = &F->c;
#define H2M_STAGE 1
#include "grdma_h2_meta_stage.inc"
#undef H2M_STAGE
}
__global__ __launch_bounds__(H2M_BLK_THREADS) void k_h2_meta_blocks(h2m_dev* F) {
  const h2m_call* const C = &F->c;
  h2m_wg* const W = F->wg;
#define H2M_STAGE 2
#include "grdma_h2_meta_stage.inc"
#undef H2M_STAGE
}
__global__ __launch_bounds__(H2M_THREADS) void k_h2_meta_emit(h2m_dev* F) {
  const h2m_call* const C = &F->c;
  h2m_wg* const W = F->wg;
  uint64_t* const R = F->res;
#define H2M_STAGE 3
#include "grdma_h2_meta_stage.inc"
#undef H2M_STAGE
}
#undef H2M_BLK
#undef H2M_NBLK
#undef H2M_LINKS

// ---- the three stages over a table of L <= H2M_LINKS_MAX links: three launches however many links.  ONE reader serves
// every link: F gives the constants (the method table, the keys, accept, rej_first, rej_n) and holds the counters; an
// entry of the table is one link's call words, its workgroups' counts and its eight result words, all three in the batch
// block of the host call (one copy up, one copy down for all links), so bad input and a cap overflow stay with their
// link.  Link l owns the workgroups [l * H2M_LINK_GRID, (l + 1) * H2M_LINK_GRID) in all three stages; its records and
// call records are its slice of the reader's scratch (the call words name it).  The counters move once for the call:
// every link's counts are complete when the blocks stage ends, so workgroup 0 of the emit launch sums them, a thread
// per link, over the links that are read (no bad block, nblocks <= meta_cap, rejections <= reject_cap: what the link's
// own workgroups decide from the same words) and bumps st_* -- by nothing where no link is read.
#define H2M_LINKS_MAX 256  // (= GRDMA_H2_BATCH_MAX, include/grdma_amd.h)
#ifdef GRDMA_WAVE_EMU
#define H2M_LINK_GRID 2
#else
#define H2M_LINK_GRID 4    // (256 links: 1024 workgroups, four to a compute unit)
#endif
struct h2m_link {
  const h2m_call* call;  // in the batch block
  h2m_wg* wg;            // H2M_LINK_GRID of them, in the batch block
  uint64_t* res;         // the item's eight words in the batch block: H2M_*
};
// (the table is written by the host in front of the launch and only read on the device: constant memory, as H2HE_ENTRY)
#ifdef GRDMA_WAVE_EMU
#define H2M_ENTRY(tab, l) ((tab)[l])
#else
#define H2M_ENTRY(tab, l) (((const __attribute__((address_space(4))) h2m_link*)(tab))[l])
#endif

#define H2M_LINKS 1
#define H2M_BLK (blockIdx.x % H2M_LINK_GRID)
#define H2M_NBLK H2M_LINK_GRID
#define H2M_OF(l)                                   \
  if ((l) >= nlinks) return; /* (uniform in the workgroup) */ \
  const h2m_call* const C = H2M_ENTRY(tab, l).call; \
  h2m_wg* const W = H2M_ENTRY(tab, l).wg;
__global__ __launch_bounds__(H2M_THREADS) void k_h2_links_meta_fields(h2m_dev* F, const h2m_link* __restrict__ tab, uint32_t nlinks) {
  if (blockIdx.x / H2M_LINK_GRID >= nlinks) return;  // (uniform in the workgroup)
  const h2m_call* const C = H2M_ENTRY(tab, blockIdx.x / H2M_LINK_GRID).call;
#define H2M_STAGE 1
#include "grdma_h2_meta_stage.inc"
#undef H2M_STAGE
}
__global__ __launch_bounds__(H2M_BLK_THREADS) void k_h2_links_meta_blocks(h2m_dev* F, const h2m_link* __restrict__ tab, uint32_t nlinks) {
  H2M_OF(blockIdx.x / H2M_LINK_GRID)
#define H2M_STAGE 2
#include "grdma_h2_meta_stage.inc"
#undef H2M_STAGE
}
__global__ __launch_bounds__(H2M_THREADS) void k_h2_links_meta_emit(h2m_dev* F, const h2m_link* __restrict__ tab, uint32_t nlinks) {
  H2M_OF(blockIdx.x / H2M_LINK_GRID)
  uint64_t* const R = H2M_ENTRY(tab, blockIdx.x / H2M_LINK_GRID).res;
#define H2M_STAGE 3
#include "grdma_h2_meta_stage.inc"
#undef H2M_STAGE
}
#undef H2M_OF
#undef H2M_BLK
#undef H2M_NBLK
#undef H2M_LINKS

}  // namespace
#endif  // GRDMA_H2_META_H
