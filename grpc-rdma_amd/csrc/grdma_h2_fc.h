// Receive flow control on the device (grdma_h2_fc): the window ledger of one transport.  The deframer's events of one
// call -> the received DATA bytes counted against the windows our SETTINGS announced, and the WINDOW_UPDATE frames that
// give them back (frame_window_update.cc: 13 bytes, length 4, type 8, flags 0, stream id, 31-bit increment), as a
// slice list of inlined slices the way grdma_h2_frame_messages writes one.  RFC 7540 6.9 with the position of the
// reference's RecvData (a frame counts where init_data_frame_parser sees its header); NOT a port of flow_control.cc:
// no BDP estimate, a fixed policy (docs/h2_deframer.md, "Receive flow control: the window ledger").
//
// Five launches of fixed shape behind the deframing; the event count is read on the device.  The keyed part (sums and
// first indices per stream) goes through a scratch table keyed by stream id -- open addressing from (id >> 1) & mask,
// as many slots as the parser's stream map, keys claimed with a compare-and-swap, values with vector atomics (add,
// min).  Kernel boundaries are the only agent-scope hand-over; inside the one-workgroup kernel barriers only.
//   k_h2_fc_clear    the scratch table, the mark words of the call's events, the call's accumulators
//   k_h2_fc_keys     per event: DATA frames add their size to the connection's sum (one atomic per wave) and, with
//                    status 0 on a stream the parser's map holds behind the call, claim the stream's slot (DATA on
//                    ids the transport never knew claims nothing: a peer cannot fill the table that way);
//                    STREAM_OPEN / STREAM_CLOSED claim it and leave their first event index there (min)
//   k_h2_fc_sums     per DATA frame with status 0: delivered to the stream's data parser when it lies in front of the
//                    stream's first STREAM_CLOSED and, for a stream opened in the call, behind its STREAM_OPEN -> the
//                    stream's sum (add) and the index of its first counted frame (min)
//   k_h2_fc_finish   one workgroup.  Per slot: a stream that neither opened nor closed in the call was delivered to
//                    only if the parser's map holds it open for reads (the deframer skips unknown and read-closed
//                    streams with status 0 too); violations; which streams get a frame.  Their first indices are
//                    marked in a bit per event, block scans over the words' popcounts give every stream its position
//                    (the order of the first counted frame); the connection's window, the caps, the result block
//   k_h2_fc_emit     fixed grid, one thread per 23-byte slice: the concatenated frames cut as grpc_slice_buffer_add
//                    merges inlined slices; writes nothing when the plan reported an overflow
// The same five stages over a table of ledgers, for the transports of a batch and the links of a group pipe
// (k_h2_links_fc_*), stand at the end of the file; both families include their bodies from csrc/grdma_h2_fc_stage.inc.
#ifndef GRDMA_H2_FC_H
#define GRDMA_H2_FC_H
#include "grdma_h2_kernels.h"

#define H2FC_THREADS 256
#define H2FC_ONE_THREADS 512
#ifdef GRDMA_WAVE_EMU
#define H2FC_GRID 2  // (the emulator runs workgroups one after another: the kernels are grid-stride)
#else
#define H2FC_GRID 256
#endif
#define H2FC_NONE 0xffffffffu
#define H2FC_MAX_INC 0x7fffffffull  // the increment is 31 bits: a larger credit is cut to it (the rest stays pending)
#define H2FC_FRAME 13ull

enum { H2FC_FRAMES = 0, H2FC_SLICES = 1, H2FC_WIRE = 2, H2FC_CONN_BYTES = 3, H2FC_STREAM_BYTES = 4, H2FC_VIOLATIONS = 5,
       H2FC_FIRST_VIOLATOR = 6, H2FC_OVERFLOW = 7 };
enum { H2FC_V_CONN = 1, H2FC_V_STREAM = 2, H2FC_V_LOST = 4 };  // GRDMA_H2_FC_* of include/grdma_amd.h

// one stream of the call
struct h2fc_slot {
  uint32_t key;     // stream id, 0 = empty
  uint32_t first;   // event index of its first counted DATA frame
  uint32_t closed;  // ... of its first STREAM_CLOSED
  uint32_t opened;  // ... of its STREAM_OPEN
  unsigned long long sum;
  uint32_t emit, pad;
};
struct h2fc_upd {
  uint32_t stream, inc;
};
// one call: where the deframer left its output
struct h2fc_call {
  const grdma_h2_event* ev;
  const grdma_h2_deframe_result* res;
  uint64_t ev_cap;
};
// the ledger, resident in HBM
struct h2fc_dev {
  const grdma_h2_parser_dev* gp;
  uint64_t stream_window, conn_window, conn_threshold, max_updates;
  uint32_t tab_mask, pad0;
  h2fc_slot* tab;
  h2fc_upd* upd;       // max_updates frames
  // scratch sized by the events of a call
  uint64_t scratch_ev;
  uint32_t* mark;      // one bit per event: the first counted frame of a stream that gets a frame
  uint32_t* mark_pre;  // per word: the marks in front of it
  // where a call writes (a standalone call sets it; a pipe's are its own tables)
  grdma_sge* out;
  uint64_t cap;
  uint8_t* hdr;
  uint64_t hdr_cap;
  // state and counters since creation
  int64_t announced;
  uint64_t lost;
  uint64_t st_calls, st_conn_bytes, st_stream_bytes, st_frames, st_conn_over, st_stream_over;
  // the call's accumulators
  unsigned long long c_conn;
  uint32_t c_full, c_pad;
  uint64_t res[8];
};

namespace {

// the events of the call a ledger can account: none when the list overflowed (k_h2_fc_finish reports it)
__device__ __forceinline__ uint64_t h2fc_events(const h2fc_dev* F, const h2fc_call* call) {
  if (call->res->overflow) return 0;
  uint64_t n = call->res->nevents;
  if (n > call->ev_cap) n = call->ev_cap;
  return n > F->scratch_ev ? 0 : n;
}
__device__ __forceinline__ bool h2fc_lost(const h2fc_dev* F, const h2fc_call* call) {
  return call->res->overflow || call->res->nevents > F->scratch_ev || F->c_full;
}

// the slot of stream id, claimed if it has none (H2FC_NONE: the table is full)
__device__ __forceinline__ uint32_t h2fc_claim(h2fc_dev* F, uint32_t id) {
  const uint32_t m = F->tab_mask;
  uint32_t s = (id >> 1) & m;
  for (uint32_t probe = 0; probe <= m; probe++, s = (s + 1) & m) {
    uint32_t k = __hip_atomic_load(&F->tab[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0 && __hip_atomic_compare_exchange_strong(&F->tab[s].key, &k, id, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT))
      return s;
    if (k == id) return s;  // (a failed exchange leaves the winner's key in k)
  }
  atomicExch(&F->c_full, 1u);
  return H2FC_NONE;
}
__device__ __forceinline__ uint32_t h2fc_find(const h2fc_dev* F, uint32_t id) {
  const uint32_t m = F->tab_mask;
  uint32_t s = (id >> 1) & m;
  for (uint32_t probe = 0; probe <= m; probe++, s = (s + 1) & m) {
    const uint32_t k = F->tab[s].key;
    if (k == id) return s;
    if (k == 0) return H2FC_NONE;
  }
  return H2FC_NONE;
}

__device__ __forceinline__ bool h2fc_is_data(const grdma_h2_event& e) { return e.kind == EV_FRAME && e.a == 0; }

// The stages' bodies are source text (csrc/grdma_h2_fc_stage.inc); the k_h2_links_fc_* kernels at the end of this file
// include the same text over a table of links.
#define H2FC_BLK blockIdx.x
#define H2FC_NBLK gridDim.x
__global__ __launch_bounds__(H2FC_THREADS) void k_h2_fc_clear(h2fc_dev* F, const h2fc_call* call) {
#define H2FC_STAGE 1
#include "grdma_h2_fc_stage.inc"
#undef H2FC_STAGE
}

__global__ __launch_bounds__(H2FC_THREADS) void k_h2_fc_keys(h2fc_dev* F, const h2fc_call* call) {
#define H2FC_STAGE 2
#include "grdma_h2_fc_stage.inc"
#undef H2FC_STAGE
}

__global__ __launch_bounds__(H2FC_THREADS) void k_h2_fc_sums(h2fc_dev* F, const h2fc_call* call) {
#define H2FC_STAGE 3
#include "grdma_h2_fc_stage.inc"
#undef H2FC_STAGE
}

__global__ __launch_bounds__(H2FC_ONE_THREADS) void k_h2_fc_finish(h2fc_dev* F, const h2fc_call* call) {
#define H2FC_STAGE 4
#include "grdma_h2_fc_stage.inc"
#undef H2FC_STAGE
}

// byte o of a frame: 24-bit length 4, type 8, flags 0, the stream id, the increment (big-endian)
__device__ __forceinline__ uint32_t h2fc_byte(uint32_t stream, uint32_t inc, uint32_t o) {
  if (o < 5) return o == 2 ? 4u : o == 3 ? 8u : 0u;
  if (o < 9) return ((stream & 0x7fffffffu) >> (8 * (8 - o))) & 0xffu;
  return ((inc & 0x7fffffffu) >> (8 * (12 - o))) & 0xffu;
}

// bytes [b0, b0 + 8) of a slice that starts r0 bytes into frame 0 of the three frames it may touch (the values travel
// as scalars: a frame picked from an array by a run-time index would live in scratch memory)
__device__ __forceinline__ uint64_t h2fc_word(uint32_t r0, uint32_t b0, uint32_t len, uint32_t s0, uint32_t i0, uint32_t s1,
                                              uint32_t i1, uint32_t s2, uint32_t i2) {
  uint64_t q = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint32_t b = b0 + j, t = r0 + b;
    const uint32_t df = t >= 26u ? 2u : t >= 13u ? 1u : 0u, o = t - 13u * df;
    const uint32_t st = df == 0 ? s0 : df == 1 ? s1 : s2, in = df == 0 ? i0 : df == 1 ? i1 : i2;
    const uint64_t v = b < len ? h2fc_byte(st, in, o) : 0u;
    q |= v << (8 * j);
  }
  return q;
}

__global__ __launch_bounds__(H2FC_THREADS) void k_h2_fc_emit(const h2fc_dev* F) {
#define H2FC_STAGE 5
#include "grdma_h2_fc_stage.inc"
#undef H2FC_STAGE
}
#undef H2FC_BLK
#undef H2FC_NBLK

// ---- the five stages over a table of L <= H2FC_LINKS_MAX links (the ledgers of a batch, the links of a group pipe):
// five launches per step however many links.  Nothing is shared between the links -- every entry has its own ledger
// block (scratch table, mark words, accumulators, result block) and its own call block -- so every atomic stays on the
// link's own h2fc_dev, and a lost call, a connection error, a cap overflow or an empty event list stay with their link.
// The entry is loaded with a uniform index: it sits in scalar registers, as the single kernels' parameters do.
//   clear, keys, sums, emit   link l owns the workgroups [l * H2FC_LINK_GRID, (l + 1) * H2FC_LINK_GRID): the single
//                             kernel's grid-stride inside that share; the share's thread 0 clears the accumulators
//   finish                    grid L: workgroup l is the one workgroup of link l -- L plans side by side
// The kernel boundary is the only agent-scope hand-over; inside the finish barriers only.
#define H2FC_LINKS_MAX 256  // (= GRDMA_H2_BATCH_MAX, include/grdma_amd.h)
#ifdef GRDMA_WAVE_EMU
#define H2FC_LINK_GRID 2
#else
#define H2FC_LINK_GRID 8    // 2048 threads per link: an event per thread up to 2048 events, grid-stride beyond
#endif
struct h2fc_link {
  h2fc_dev* F;
  const h2fc_call* call;
};
// A pointer read from the table is, to the compiler, a generic one: every access through it would be a flat instruction
// with the address in a VGPR pair, where the single kernels' parameters (known to be global) stay in scalar registers.
// The table is written by the host in front of the launch and only read on the device, so it is read as constant
// memory: pointers loaded from there are taken as global ones, and the link kernels address as their single twins do.
#ifdef GRDMA_WAVE_EMU
#define H2FC_ENTRY(tab, l) ((tab)[l])
#else
#define H2FC_ENTRY(tab, l) (((const __attribute__((address_space(4))) h2fc_link*)(tab))[l])
#endif

// (a link's share of the grid)
#define H2FC_BLK (blockIdx.x % H2FC_LINK_GRID)
#define H2FC_NBLK H2FC_LINK_GRID
__global__ __launch_bounds__(H2FC_THREADS) void k_h2_links_fc_clear(const h2fc_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2FC_LINK_GRID;
  if (l >= nlinks) return;
  h2fc_dev* const F = H2FC_ENTRY(tab, l).F;
  const h2fc_call* const call = H2FC_ENTRY(tab, l).call;
#define H2FC_STAGE 1
#include "grdma_h2_fc_stage.inc"
#undef H2FC_STAGE
}

__global__ __launch_bounds__(H2FC_THREADS) void k_h2_links_fc_keys(const h2fc_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2FC_LINK_GRID;
  if (l >= nlinks) return;
  h2fc_dev* const F = H2FC_ENTRY(tab, l).F;
  const h2fc_call* const call = H2FC_ENTRY(tab, l).call;
#define H2FC_STAGE 2
#include "grdma_h2_fc_stage.inc"
#undef H2FC_STAGE
}

__global__ __launch_bounds__(H2FC_THREADS) void k_h2_links_fc_sums(const h2fc_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2FC_LINK_GRID;
  if (l >= nlinks) return;
  h2fc_dev* const F = H2FC_ENTRY(tab, l).F;
  const h2fc_call* const call = H2FC_ENTRY(tab, l).call;
#define H2FC_STAGE 3
#include "grdma_h2_fc_stage.inc"
#undef H2FC_STAGE
}

__global__ __launch_bounds__(H2FC_ONE_THREADS) void k_h2_links_fc_finish(const h2fc_link* __restrict__ tab) {
  h2fc_dev* const F = H2FC_ENTRY(tab, blockIdx.x).F;
  const h2fc_call* const call = H2FC_ENTRY(tab, blockIdx.x).call;
#define H2FC_STAGE 4
#include "grdma_h2_fc_stage.inc"
#undef H2FC_STAGE
}

__global__ __launch_bounds__(H2FC_THREADS) void k_h2_links_fc_emit(const h2fc_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2FC_LINK_GRID;
  if (l >= nlinks) return;
  const h2fc_dev* const F = H2FC_ENTRY(tab, l).F;
#define H2FC_STAGE 5
#include "grdma_h2_fc_stage.inc"
#undef H2FC_STAGE
}
#undef H2FC_BLK
#undef H2FC_NBLK

}  // namespace
#endif  // GRDMA_H2_FC_H
