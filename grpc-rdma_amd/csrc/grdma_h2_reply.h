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
// The many-link forms k_h2_reply_plan_links / k_h2_reply_emit_links (a table of framers: the replies of a batch, the
// links of a group reply pipe) are at the end of this file; the plan's body is one source text for both plan kernels,
// csrc/grdma_h2_reply_plan.inc.
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
#include "grdma_h2_reply_plan.inc"
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

// ---- the two kernels over a table of L <= H2R_LINKS_MAX links (replies of a batch, links of a group reply pipe): two
// launches however many links.  Nothing is shared between the links -- every entry has its own h2r_dev, scratch, source
// assembler and targets -- so an overflow, a shape mismatch or a skipped assembler call stay with their link.  The entry
// is loaded with a uniform index: it sits in scalar registers, as the single kernels' parameter does.
//   plan   grid L: workgroup l is the one plan workgroup of link l -- L plans side by side
//   emit   a fixed grid; the messages of ALL links by one static grid-stride, so an idle or failed link idles nobody:
//          every workgroup builds the exclusive prefix of the links' kept counts in LDS (one block scan; a link whose
//          result block reports an overflow contributes 0), a wave finds the link of its message by binary search over
//          it (wave-uniform: the link's pointers stay scalar) and lays the message out with that link's tables
// The kernel boundary is the only agent-scope hand-over; inside a workgroup barriers only.
#define H2R_LINKS_MAX 256  // (= GRDMA_H2_BATCH_MAX, include/grdma_amd.h; one thread per link in the emit's block scan)
struct h2r_link {
  h2r_dev* R;
};
static_assert(H2R_LINKS_MAX <= H2_EMIT_THREADS, "k_h2_reply_emit_links scans one link per thread");

__global__ __launch_bounds__(PLAN_THREADS) void k_h2_reply_plan_links(const h2r_link* __restrict__ tab) {
  h2r_dev* const R = tab[blockIdx.x].R;
#include "grdma_h2_reply_plan.inc"
}

__global__ __launch_bounds__(H2_EMIT_THREADS) void k_h2_reply_emit_links(const h2r_link* __restrict__ tab, uint32_t nlinks) {
  __shared__ uint64_t s_pre[H2R_LINKS_MAX + 1];  // exclusive prefix of the links' kept messages; [nlinks]: the total
  __shared__ uint64_t s_wave[H2_EMIT_THREADS / 64];
  const int lane = threadIdx.x & 63;
  const uint32_t wv = uni32(threadIdx.x >> 6);
  uint64_t mine = 0;
  if (threadIdx.x < nlinks) {
    const h2r_dev* const R = tab[threadIdx.x].R;
    if (!R->res[H2R_OVERFLOW]) mine = R->res[H2R_KEPT];
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
  const uint64_t waves = (uint64_t)gridDim.x * (H2_EMIT_THREADS / 64);
  for (uint64_t g = (uint64_t)blockIdx.x * (H2_EMIT_THREADS / 64) + wv; g < T; g += waves) {
    uint32_t ll = 0, lh = nlinks;  // the last link whose prefix <= g (a link without messages shares its prefix with the next)
    while (lh - ll > 1) {
      const uint32_t mid = (ll + lh) / 2;
      if (uni64(s_pre[mid]) <= g) ll = mid;
      else lh = mid;
    }
    const h2r_dev* const R = tab[ll].R;
    const uint64_t i = g - uni64(s_pre[ll]);
    h2_emit_message(R->msgs, i, R->res[H2R_KEPT], R->max_frame, R->out, R->cap, R->hdr, R->hdr_cap, R->pos[i], lane);
  }
}

}  // namespace
#endif  // GRDMA_H2_REPLY_H
