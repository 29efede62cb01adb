// Control replies on the device (grdma_h2_ctl, "the control-reply writer"): the frames HTTP/2 obliges a transport to
// answer, written from the deframer's events with no host step in between -- a SETTINGS ACK for every SETTINGS frame of
// the peer (RFC 7540 6.5.3), a PING ACK with the same 8 bytes for every PING (6.7), RST_STREAM(PROTOCOL_ERROR) for every
// stream error the deframer reports (the status byte of a FRAME event, or the 0xff pseudo frame) -- and a record of what
// the peer said: its SETTINGS ACKs, its PING ACKs with the last opaque value, its GOAWAYs.  The rules stand in
// include/grdma_amd.h ("Control replies"); the sequential reference is tests/h2_control_model.py.
//
// Order of the output: the PING ACKs first, then SETTINGS ACKs and RST_STREAMs in the order of their events.  RFC 7540
// fixes no order between these replies; this one is a FIXED CHOICE (the reference transport flushes its ping acks in
// front of the buffer its other control frames are queued in, when it begins a write).
//
// Frames of a connection follow one another, so the order of the frames' completions is the order of their FRAME events
// with the carried frame (the one the previous call's end cut) in front, and only the LAST frame of a call can be open at
// its end: the frame behind whose FRAME event stands neither another frame nor a PAYLOAD event with is_last.  That is
// what makes every walk short: no thread looks for the end of its frame, a PING or GOAWAY thread reads the PAYLOAD
// events of its first 8 bytes and stops.
//
// Four launches of fixed shape behind a deframing (the event count is read on the device).  In the grid stages a
// workgroup owns a CONTIGUOUS share of the events, so block order is event order:
//   k_h2_ctl_last    per workgroup the position of its last FRAME event (the 0xff pseudo frames are none) and of its last
//                    PAYLOAD event with is_last; the first thread clears the outgoing carry
//   k_h2_ctl_mark    every workgroup takes the maximum of the 256 positions: the call's last frame and whether it is
//                    complete.  One thread per FRAME event classifies its frame, a PING or GOAWAY thread gathers the 8
//                    bytes from the receive arena; the open frame becomes the outgoing carry.  Per workgroup the counts
//                    of PING replies, queued replies and queued bytes, of what the peer said, and its last PING ACK and
//                    GOAWAY.  The grid's first thread continues the carried frame.
//   k_h2_ctl_scan    one workgroup: exclusive scan of the workgroups' counts, the caps, the result block; unless a cap
//                    overflowed the carry, the peer's record and the counters are committed
//   k_h2_ctl_emit    recomputes each reply's rank inside its workgroup with a block scan per 256 events and writes its
//                    bytes at its offset -- 17 x rank for a PING ACK, 17 x pings + the earlier queued bytes for the
//                    others -- then the slice descriptors of the 23-byte cuts; nothing after an overflow
// Kernel boundaries are the only agent-scope hand-over; inside a workgroup barriers and LDS atomics.  No global atomic at
// all: the order comes from prefix sums over event positions.
// The same four stages over a table of links (k_h2_links_ctl_*) stand at the end of the file; both families include their
// bodies from csrc/grdma_h2_ctl_stage.inc.
#ifndef GRDMA_H2_CTL_H
#define GRDMA_H2_CTL_H
#include "grdma_h2_kernels.h"

#define H2CTL_THREADS 256
#ifdef GRDMA_WAVE_EMU
#define H2CTL_GRID 2  // (the emulator runs workgroups one after another)
#else
#define H2CTL_GRID 256
#endif
#define H2CTL_GRID_MAX 256  // (one thread per workgroup in the scan)
#define H2CTL_PING 17u
#define H2CTL_SETTINGS_ACK 9u
#define H2CTL_RST 13u

enum { H2CTL_FRAMES = 0, H2CTL_SLICES = 1, H2CTL_WIRE = 2, H2CTL_N_SETTINGS = 3, H2CTL_N_PING = 4, H2CTL_N_RST = 5, H2CTL_FLAGS = 6,
       H2CTL_OVERFLOW = 7 };
enum { H2CTL_F_LOST = 1, H2CTL_F_GOAWAY = 2 };  // GRDMA_H2_CTL_* of include/grdma_amd.h
// what a FRAME event asks for
enum { H2CTL_K_NONE = 0, H2CTL_K_PING = 1, H2CTL_K_SETTINGS = 2, H2CTL_K_RST = 3, H2CTL_K_GOT_SETTINGS_ACK = 4, H2CTL_K_GOT_PING_ACK = 5,
       H2CTL_K_GOT_GOAWAY = 6, H2CTL_K_OPEN = 7 };

// a control frame in flight: what a thread holds of its frame, and what a call's end leaves behind
struct h2ctl_frame {
  uint32_t type;    // 4 SETTINGS, 6 PING, 7 GOAWAY, 0 none
  uint32_t flags;
  uint32_t nbytes;  // of the first 8 payload bytes (PING, GOAWAY): how many are in
  uint32_t pad;
  uint64_t acc;     // those bytes, big-endian
};
// one call: where the deframer left its output and what it read
struct h2ctl_call {
  const grdma_h2_event* ev;
  const grdma_h2_deframe_result* res;
  const grdma_slice_out* sl;
  const uint8_t* arena;
  uint64_t ev_cap, nsl;
  uint64_t skipped;  // a standalone deframing in front of this one was never taken in
};
// what one workgroup hands to the scan
struct h2ctl_blk {
  uint32_t last_frame, last_done;  // positions (event index + 1, 0 = none) in the workgroup's share
  uint32_t pings, queued, rsts;    // replies
  uint32_t got_settings_acks, got_ping_acks, got_goaways;
  uint64_t qbytes;                 // bytes of the queued replies
  uint32_t pa_pos, ga_pos;         // the share's last PING ACK / GOAWAY received, 0 = none
  uint64_t pa_acc, ga_acc;
  uint64_t pre_pings, pre_qbytes;  // the scan's: replies of the workgroups in front
};
// the writer, resident in HBM
struct h2ctl_dev {
  // where a call writes (the host sets it)
  grdma_sge* out;
  uint64_t cap;
  uint8_t* hdr;
  uint64_t hdr_cap;
  // state and counters since creation (the device's)
  uint64_t max_replies;
  h2ctl_frame carry, carry_out;
  uint32_t lost, pad0;
  uint64_t peer[8];
  uint64_t st_calls, st_settings_acks, st_ping_acks, st_rsts, st_wire;
  // a call's scratch
  uint32_t c_kind, pad1;  // what the carried frame asks for (H2CTL_K_*)
  uint64_t c_acc;
  uint32_t last_frame, last_done;
  uint64_t res[8];  // H2CTL_*
  h2ctl_blk blk[H2CTL_GRID_MAX];
};

namespace {

__device__ __forceinline__ bool h2ctl_lost(const h2ctl_call* call) { return call->res->overflow || call->res->nevents > call->ev_cap; }
__device__ __forceinline__ bool h2ctl_taken(const h2ctl_call* call) { return !h2ctl_lost(call) && call->res->error == 0; }

// The first 8 payload bytes of f over the PAYLOAD events from j on: bounded by the event count, by the frame's end and
// by 8 bytes.
__device__ __forceinline__ void h2ctl_gather(const h2ctl_call* call, h2ctl_frame& f, uint64_t j, uint64_t n) {
  for (; j < n && f.nbytes < 8; j++) {
    const grdma_h2_event pe = call->ev[j];
    if (pe.kind != EV_PAYLOAD) return;
    if (pe.slice < call->nsl) {
      const grdma_slice_out sl = call->sl[pe.slice];
      if ((uint64_t)pe.a + pe.b <= sl.len) {
        const uint8_t* src = call->arena + sl.off + pe.a;
        for (uint32_t k = 0; k < pe.b && f.nbytes < 8; k++) {
          f.acc = (f.acc << 8) | src[k];
          f.nbytes++;
        }
      }
    }
    if (pe.c) return;
  }
}

// what a complete frame asks for
__device__ __forceinline__ uint32_t h2ctl_kind(const h2ctl_frame& f) {
  if (f.type == FT_SETTINGS) return (f.flags & 1u) ? H2CTL_K_GOT_SETTINGS_ACK : H2CTL_K_SETTINGS;
  if (f.type == FT_PING) return (f.flags & 1u) ? H2CTL_K_GOT_PING_ACK : H2CTL_K_PING;
  return f.type == FT_GOAWAY ? H2CTL_K_GOT_GOAWAY : H2CTL_K_NONE;
}

// The event at index i: what it asks for, with its frame in f (stream: the RST_STREAM's).  last_frame / last_done: the
// positions of the call's last FRAME event and last PAYLOAD event with is_last.
__device__ __forceinline__ uint32_t h2ctl_classify(const h2ctl_call* call, uint64_t i, uint64_t n, uint32_t last_frame, uint32_t last_done,
                                                   h2ctl_frame& f, uint32_t& stream) {
  const grdma_h2_event e = call->ev[i];
  if (e.kind != EV_FRAME) return H2CTL_K_NONE;
  if (e.a == 0xffu || (e.b >> 8) != 0) {  // a stream error: the pseudo frame inside a DATA payload, or the status byte
    stream = e.c;
    return H2CTL_K_RST;
  }
  if (e.a != FT_SETTINGS && e.a != FT_PING && e.a != FT_GOAWAY) return H2CTL_K_NONE;
  f.type = e.a;
  f.flags = e.b & 0xffu;
  f.nbytes = 0;
  f.pad = 0;
  f.acc = 0;
  if (e.a != FT_SETTINGS) h2ctl_gather(call, f, i + 1, n);
  const uint32_t v = (uint32_t)i + 1u;
  if (v == last_frame && last_done <= last_frame) return H2CTL_K_OPEN;  // the call's end cut it
  return h2ctl_kind(f);
}

// byte o of the output: slice o / 23, 32 bytes of arena a slice
__device__ __forceinline__ void h2ctl_put(uint8_t* hdr, uint64_t o, uint32_t byte) {
  const uint64_t k = o / H2_INLINED;
  hdr[32 * k + (o - k * H2_INLINED)] = (uint8_t)byte;
}
// a frame of len <= 17 bytes at offset o: bytes 0..7 are w0, 8..15 w1 (big-endian words), byte 16 is b16
__device__ __forceinline__ void h2ctl_write(uint8_t* hdr, uint64_t o, uint64_t w0, uint64_t w1, uint32_t b16, uint32_t len) {
  for (uint32_t k = 0; k < len; k++) {
    const uint32_t b = k < 8 ? (uint32_t)(w0 >> (56 - 8 * k)) : k < 16 ? (uint32_t)(w1 >> (56 - 8 * (k - 8))) : b16;
    h2ctl_put(hdr, o + k, b & 0xffu);
  }
}
__device__ __forceinline__ void h2ctl_write_reply(uint8_t* hdr, uint64_t o, uint32_t kind, uint64_t acc, uint32_t stream) {
  if (kind == H2CTL_K_PING) h2ctl_write(hdr, o, 0x0000080601000000ull, acc >> 8, (uint32_t)acc, H2CTL_PING);
  else if (kind == H2CTL_K_SETTINGS) h2ctl_write(hdr, o, 0x0000000401000000ull, 0, 0, H2CTL_SETTINGS_ACK);
  else h2ctl_write(hdr, o, 0x0000040300000000ull | (stream >> 8), ((uint64_t)(stream & 0xffu) << 56) | (1ull << 24), 0, H2CTL_RST);
}

__device__ __forceinline__ uint64_t h2ctl_bswap(uint64_t v) { return __builtin_bswap64(v); }

// The stages' bodies are source text (csrc/grdma_h2_ctl_stage.inc); the k_h2_links_ctl_* kernels below include the same
// text over a table of links.  H2CTL_NBLK is the grid of the grid stages -- the scan, one workgroup, reads that many
// blocks of counts -- so it is a constant, not gridDim.x.
#define H2CTL_BLK blockIdx.x
#define H2CTL_NBLK H2CTL_GRID
__global__ __launch_bounds__(H2CTL_THREADS) void k_h2_ctl_last(h2ctl_dev* F, const h2ctl_call* call) {
#define H2CTL_STAGE 1
#include "grdma_h2_ctl_stage.inc"
#undef H2CTL_STAGE
}

__global__ __launch_bounds__(H2CTL_THREADS) void k_h2_ctl_mark(h2ctl_dev* F, const h2ctl_call* call) {
#define H2CTL_STAGE 2
#include "grdma_h2_ctl_stage.inc"
#undef H2CTL_STAGE
}

__global__ __launch_bounds__(H2CTL_THREADS) void k_h2_ctl_scan(h2ctl_dev* F, const h2ctl_call* call) {
#define H2CTL_STAGE 3
#include "grdma_h2_ctl_stage.inc"
#undef H2CTL_STAGE
}

__global__ __launch_bounds__(H2CTL_THREADS) void k_h2_ctl_emit(h2ctl_dev* F, const h2ctl_call* call) {
#define H2CTL_STAGE 4
#include "grdma_h2_ctl_stage.inc"
#undef H2CTL_STAGE
}
#undef H2CTL_BLK
#undef H2CTL_NBLK

// ---- the four kernels over a table of L <= H2CTL_LINKS_MAX links: four launches however many links.  Nothing is shared
// between the links: every entry has its own h2ctl_dev (carry, record, counters, the workgroups' counts, result block)
// and its own call block, so a lost call, a connection error, a skipped deframing, a cap overflow or an empty event list
// stay with their link.  In the grid stages link l owns the workgroups [l * H2CTL_LINK_GRID, (l + 1) * H2CTL_LINK_GRID):
// its events in that many contiguous shares; the scan runs one workgroup per link.
#define H2CTL_LINKS_MAX 256  // (= GRDMA_H2_BATCH_MAX, include/grdma_amd.h)
#ifdef GRDMA_WAVE_EMU
#define H2CTL_LINK_GRID 2
#else
#define H2CTL_LINK_GRID 8    // (H2SW_LINK_GRID's sizing: 2048 threads per link)
#endif
struct h2ctl_link {
  h2ctl_dev* F;
  const h2ctl_call* call;
};
// (the table is written by the host in front of the launch and only read on the device: constant memory, as H2SW_ENTRY)
#ifdef GRDMA_WAVE_EMU
#define H2CTL_ENTRY(tab, l) ((tab)[l])
#else
#define H2CTL_ENTRY(tab, l) (((const __attribute__((address_space(4))) h2ctl_link*)(tab))[l])
#endif

#define H2CTL_BLK (blockIdx.x % H2CTL_LINK_GRID)
#define H2CTL_NBLK H2CTL_LINK_GRID
__global__ __launch_bounds__(H2CTL_THREADS) void k_h2_links_ctl_last(const h2ctl_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2CTL_LINK_GRID;
  if (l >= nlinks) return;
  h2ctl_dev* const F = H2CTL_ENTRY(tab, l).F;
  const h2ctl_call* const call = H2CTL_ENTRY(tab, l).call;
#define H2CTL_STAGE 1
#include "grdma_h2_ctl_stage.inc"
#undef H2CTL_STAGE
}

__global__ __launch_bounds__(H2CTL_THREADS) void k_h2_links_ctl_mark(const h2ctl_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2CTL_LINK_GRID;
  if (l >= nlinks) return;
  h2ctl_dev* const F = H2CTL_ENTRY(tab, l).F;
  const h2ctl_call* const call = H2CTL_ENTRY(tab, l).call;
#define H2CTL_STAGE 2
#include "grdma_h2_ctl_stage.inc"
#undef H2CTL_STAGE
}

__global__ __launch_bounds__(H2CTL_THREADS) void k_h2_links_ctl_scan(const h2ctl_link* __restrict__ tab) {
  h2ctl_dev* const F = H2CTL_ENTRY(tab, blockIdx.x).F;
  const h2ctl_call* const call = H2CTL_ENTRY(tab, blockIdx.x).call;
#define H2CTL_STAGE 3
#include "grdma_h2_ctl_stage.inc"
#undef H2CTL_STAGE
}

__global__ __launch_bounds__(H2CTL_THREADS) void k_h2_links_ctl_emit(const h2ctl_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2CTL_LINK_GRID;
  if (l >= nlinks) return;
  h2ctl_dev* const F = H2CTL_ENTRY(tab, l).F;
  const h2ctl_call* const call = H2CTL_ENTRY(tab, l).call;
#define H2CTL_STAGE 4
#include "grdma_h2_ctl_stage.inc"
#undef H2CTL_STAGE
}
#undef H2CTL_BLK
#undef H2CTL_NBLK

}  // namespace
#endif  // GRDMA_H2_CTL_H
