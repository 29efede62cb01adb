// Replies framed from received-message descriptors (grdma_h2_reply): the descriptors the message assembler left on
// the device (h2a_dev::desc / ndesc, csrc/grdma_h2_asm.h) -> the slice list grpc_endpoint_write would receive for the
// same messages sent back (echo) or on to another stream (a proxy), with no host step in between.  The wire is what
// grdma_h2_frame_messages yields for the kept messages in descriptor order: grpc_chttp2_encode_data plus the 5-byte
// message header on one outbuf (frame_data.cc:64-90, chttp2_transport.cc:1502-1510); payload goes by reference into
// the assembler's arena.
//
// Two launches of fixed shape; the descriptor count is read from device memory, as the assembler's kernels read the
// event count.  The plan's global stores are read by the next launch: the kernel boundary is the hand-over.  Inside the
// plan workgroup the hand-overs are barriers.
//   k_h2_reply_plan   one workgroup.  Descriptors in blocks of the workgroup's size: kept (status OK, and routed when
//                     there is a route table: binary search over the table sorted by from_stream) or dropped; the kept
//                     ones compacted with a block scan into a grdma_h2_msg_dev table (payload = arena + offset, the
//                     routed stream id, the compressed flag; never END_STREAM).  Then, over the COMPACTED table, the
//                     index of k_h2_frame_index: h2_msg_size per message and block scans -> slice slot, header-arena
//                     offset, totals.  A dropped descriptor does not exist for the layout: the inlined-slice merge
//                     behind a run of empty messages sees the compacted neighbours.
//   k_h2_reply_emit   fixed grid.  Waves take messages by static grid-stride (wave w: messages w, w + W, ...) and lay
//                     each one out with h2_emit_message.  Writes nothing when the plan reported an overflow or, in a
//                     pipe, a shape other than the one the job's graph was recorded for.
#ifndef GRDMA_H2_REPLY_H
#define GRDMA_H2_REPLY_H
#include "grdma_h2_asm.h"

#ifdef GRDMA_WAVE_EMU
#define H2R_GRID 2  // (the emulator runs workgroups one after another: the kernel is grid-stride)
#else
#define H2R_GRID 256
#endif
#define H2R_MAX_ROUTES 4096u

enum { H2R_KEPT = 0, H2R_DROPPED_STATUS = 1, H2R_UNROUTED = 2, H2R_SLICES = 3, H2R_HDR_BYTES = 4, H2R_WIRE_BYTES = 5,
       H2R_OVERFLOW = 6 };

// the reply framer, resident in HBM
struct h2r_dev {
  const h2a_dev* src;              // the assembler whose last call is framed
  const grdma_h2_route* routes;    // sorted by from_stream; n_routes = 0: every message goes out on its own stream
  uint32_t n_routes, max_frame;
  uint64_t max_messages;           // descriptors of one call, at most (capacity of msgs / pos)
  grdma_h2_msg_dev* msgs;          // the kept messages, compacted
  grdma_h2_msg_pos* pos;
  // where a call frames to (a standalone call sets it; a pipe's is its job's slice table)
  grdma_sge* out;
  uint64_t cap;
  uint8_t* hdr;
  uint64_t hdr_cap;
  // a pipe: the shape the job's graph was recorded for (check_shape = 1)
  uint64_t check_shape, want_slices, want_wire;
  // the result block (H2R_*); overflow: 1 = a cap, 2 = not the recorded shape
  uint64_t res[8];
};

namespace {

// the stream a message received on `id` goes out on (0: unrouted)
__device__ __forceinline__ uint32_t h2r_route(const h2r_dev* R, uint32_t id) {
  if (R->n_routes == 0) return id;
  uint32_t lo = 0, hi = R->n_routes;  // the first entry whose from_stream >= id
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (R->routes[mid].from_stream < id) lo = mid + 1;
    else hi = mid;
  }
  if (lo < R->n_routes && R->routes[lo].from_stream == id) return R->routes[lo].to_stream;
  return 0;
}

__global__ __launch_bounds__(PLAN_THREADS) void k_h2_reply_plan(h2r_dev* R) {
  __shared__ uint64_t s_wave[PLAN_THREADS / 64];
  const h2a_dev* A = R->src;
  const uint64_t tid = threadIdx.x;
  // (a call the assembler skipped left no descriptors; more than the tables hold: nothing is framed)
  const bool bad = A->skip != 0 || A->ndesc > A->desc_cap || A->ndesc > R->max_messages;
  const uint64_t nd = bad ? 0 : A->ndesc;
  const grdma_h2_rx_msg* desc = A->desc;
  grdma_h2_msg_dev* msgs = R->msgs;
  // 1. kept or dropped, the kept ones compacted in descriptor order
  uint64_t kept = 0, my_status = 0, my_unrouted = 0;
  for (uint64_t d0 = 0; d0 < nd; d0 += PLAN_THREADS) {
    const uint64_t i = d0 + tid;
    uint64_t keep = 0;
    grdma_h2_msg_dev m{nullptr, 0, 0, 0};
    if (i < nd) {
      const grdma_h2_rx_msg d = desc[i];
      if (d.status != GRDMA_H2_MSG_OK) {
        my_status++;
      } else {
        const uint32_t to = h2r_route(R, d.stream_id);
        if (to == 0) {
          my_unrouted++;
        } else {
          keep = 1;
          m.payload = A->arena + d.offset;
          m.len = d.length;
          m.stream_id = to;
          m.flags = d.flags & 1;
        }
      }
    }
    uint64_t tot;
    const uint64_t x = block_excl_scan(keep, s_wave, &tot);
    if (keep) msgs[kept + x] = m;
    kept += tot;
  }
  uint64_t n_status, n_unrouted;
  block_excl_scan(my_status, s_wave, &n_status);
  block_excl_scan(my_unrouted, s_wave, &n_unrouted);
  __syncthreads();  // the compacted table is complete: sizes look at a message's neighbours
  // 2. sizes and positions over the compacted table (the loop of k_h2_frame_index)
  const uint32_t max_frame = R->max_frame;
  uint64_t base_sl = 0, base_hdr = 0, base_wire = 0;
  for (uint64_t m0 = 0; m0 < kept; m0 += PLAN_THREADS) {
    const uint64_t i = m0 + tid;
    uint64_t n_sl = 0, n_hdr = 0, n_wire = 0;
    uint32_t mode = 0;
    if (i < kept) h2_msg_size(msgs, i, max_frame, &n_sl, &n_hdr, &n_wire, &mode);
    uint64_t tot_sl, tot_hdr, tot_wire;
    const uint64_t x_sl = block_excl_scan(n_sl, s_wave, &tot_sl);
    const uint64_t x_hdr = block_excl_scan(n_hdr, s_wave, &tot_hdr);
    block_excl_scan(n_wire, s_wave, &tot_wire);
    if (i < kept) {
      grdma_h2_msg_pos q;
      q.sl = base_sl + x_sl;
      q.hdr = base_hdr + x_hdr;
      q.mode = mode;
      q.pad = 0;
      R->pos[i] = q;
    }
    base_sl += tot_sl;
    base_hdr += tot_hdr;
    base_wire += tot_wire;
  }
  if (tid == 0) {
    uint64_t overflow = (bad || base_sl > R->cap || base_hdr > R->hdr_cap) ? 1 : 0;
    if (!bad && R->check_shape && (base_sl != R->want_slices || base_wire != R->want_wire)) overflow = 2;
    R->res[H2R_KEPT] = kept;
    R->res[H2R_DROPPED_STATUS] = n_status;
    R->res[H2R_UNROUTED] = n_unrouted;
    R->res[H2R_SLICES] = base_sl;
    R->res[H2R_HDR_BYTES] = base_hdr;
    R->res[H2R_WIRE_BYTES] = base_wire;
    R->res[H2R_OVERFLOW] = overflow;
  }
}

__global__ __launch_bounds__(H2_EMIT_THREADS) void k_h2_reply_emit(const h2r_dev* R) {
  if (R->res[H2R_OVERFLOW]) return;  // (nothing half-written in front of a job; a standalone call fails)
  const uint64_t n = R->res[H2R_KEPT];
  const int lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (H2_EMIT_THREADS / 64);
  const grdma_h2_msg_dev* msgs = R->msgs;
  const grdma_h2_msg_pos* pos = R->pos;
  const uint32_t max_frame = R->max_frame;
  grdma_sge* out = R->out;
  uint8_t* hdr = R->hdr;
  const uint64_t cap = R->cap, hdr_cap = R->hdr_cap;
  for (uint64_t i = (uint64_t)blockIdx.x * (H2_EMIT_THREADS / 64) + (threadIdx.x >> 6); i < n; i += waves)
    h2_emit_message(msgs, i, n, max_frame, out, cap, hdr, hdr_cap, pos[i], lane);
}

}  // namespace
#endif  // GRDMA_H2_REPLY_H
