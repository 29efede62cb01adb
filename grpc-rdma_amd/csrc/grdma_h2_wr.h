// Replies under the peer's windows (the "windowed reply"): the descriptors the message assembler left on the device
// (csrc/grdma_h2_asm.h), routed as grdma_h2_reply routes them (csrc/grdma_h2_reply.h), framed under the send windows of
// the transport they go out on (grdma_h2_sw, csrc/grdma_h2_sw.h) -- and what the windows cut off waits in a queue in
// device memory, its payload unreleased in the assembler's ring, until a later call frames it in front of what has
// arrived since.  No host step sees a descriptor (docs/h2_deframer.md, "Replies under the peer's windows"; the rules:
// include/grdma_amd.h).
//
// The queue: two tables of max_pending entries that change roles (as the send windows' stream tables do) -- per entry
// the message (grdma_h2_msg_dev: payload in the assembler's arena, outgoing stream, compressed flag), the
// flow-controlled bytes already sent, and the report rank of its descriptor (rank_base + index: the unit
// k_h2_asm_release counts in, so a descriptor without a record -- NO_SPACE -- counts as every other).  The progress
// words are the queue's own: the plan's prog_out belongs to h2sw_dev and a grdma_h2_sw_frame call between two windowed
// replies overwrites it.
//
// A call, four launches of fixed shape:
//   k_h2_wr_queue    one workgroup.  The current table's entries that are unfinished and whose outgoing stream the map
//                    of the send windows' parser still holds, compacted with block scans into the other table; behind
//                    them the kept descriptors of the source assembler's last call (status OK, routed, stream live),
//                    progress 0.  It points the send windows' framing words at that table and writes the message
//                    count THERE: the host does not know it.  More entries than max_pending, a skipped assembler call
//                    or more descriptors than the reply holds: the count is 0, the plan frames nothing.
//   k_h2_sw_plan, k_h2_sw_emit   unchanged, over that table
//   k_h2_wr_commit   one workgroup.  Unless something overflowed: the plan's progress goes into the queue's own words
//                    and the tables change roles.  Either way: how many entries of the table that is current behind the
//                    call are unfinished, the smallest rank among them (ranks ascend along the queue: a reduction, not
//                    a search), `releasable`, the result block.
// Kernel boundaries are the only agent-scope hand-over; inside a workgroup barriers only.  The same two bodies over a
// table of links (k_h2_links_wr_*: workgroup l is link l) stand at the end of the file; both families include
// csrc/grdma_h2_wr_stage.inc.
#ifndef GRDMA_H2_WR_H
#define GRDMA_H2_WR_H
#include "grdma_h2_reply.h"
#include "grdma_h2_sw.h"

// Both stages are one workgroup of H2WR_THREADS: a table of the flagship step's size (1008 messages) is one block of
// the scans, so the dependent loads of an entry (descriptor, route, stream map) are waited for once, not four times.
#define H2WR_THREADS 1024

// the result block (GRDMA_H2_WR_* of include/grdma_amd.h)
enum { H2WR_FINISHED = 0, H2WR_PENDING = 1, H2WR_SLICES = 2, H2WR_HDR = 3, H2WR_WIRE = 4, H2WR_GRANTED = 5, H2WR_STALL = 6,
       H2WR_OVERFLOW = 7, H2WR_TAKEN = 8, H2WR_DROPPED_STATUS = 9, H2WR_UNROUTED = 10, H2WR_CLOSED = 11, H2WR_RELEASABLE = 12,
       H2WR_FLAGS = 13, H2WR_US = 14, H2WR_SPARE = 15 };
enum { H2WR_FLAG_LOST = 1 };

// the queue of one reply framer, resident in HBM
struct h2wr_dev {
  const h2r_dev* R;            // routes, source assembler, max_messages
  h2sw_dev* F;                 // the send windows the replies go out under
  grdma_h2_msg_dev* msgs[2];   // max_pending entries each
  uint64_t* prog[2];           // flow-controlled bytes sent, per entry
  uint64_t* rank[2];           // report rank of the entry's descriptor
  uint32_t max_pending, cur;
  uint64_t nq;                 // entries of table `cur` (finished ones among them until the next call compacts)
  uint64_t lost;               // sticky: a source call was never taken
  // a call (the host sets it)
  uint64_t take;               // the source assembler's last call is new: append its kept descriptors
  uint64_t untaken;            // ... is new but stays where it is (PENDING_ONLY): not releasable
  uint64_t lost_now;           // the count of source calls ran ahead by more than one
  // what k_h2_wr_queue found
  uint64_t n_tab, n_new, n_status, n_unrouted, n_closed, count, over;  // over: 1 = the source call, 2 = the queue is full
  uint64_t res[16];            // H2WR_*
};

namespace {

// exclusive scan of one value per thread over the workgroup; returns the prefix and, in *total, the sum
__device__ __forceinline__ uint64_t h2wr_block_scan(uint64_t v, uint64_t* ws, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t incl = wave_incl_scan(v, lane);
  if (lane == 63) ws[wave] = incl;
  __syncthreads();
  uint64_t base = 0, tot = 0;
  for (int w = 0; w < H2WR_THREADS / 64; w++) {
    const uint64_t sum = ws[w];
    if (w < wave) base += sum;
    tot += sum;
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

#define H2WR_STAGE 1
__global__ __launch_bounds__(H2WR_THREADS) void k_h2_wr_queue(h2wr_dev* W) {
#include "grdma_h2_wr_stage.inc"
}
#undef H2WR_STAGE

#define H2WR_STAGE 2
__global__ __launch_bounds__(H2WR_THREADS) void k_h2_wr_commit(h2wr_dev* W) {
#include "grdma_h2_wr_stage.inc"
}
#undef H2WR_STAGE

// ---- the two kernels over a table of L <= H2WR_LINKS_MAX links: workgroup l is the one workgroup of link l, so a batch
// is four launches however many links (k_h2_links_sw_plan and k_h2_links_sw_emit run unchanged between them).  Nothing
// is shared between the links: an overflow, a full queue or a lost call stay with their link.  The entry is loaded with a
// uniform index from constant memory, as H2SW_ENTRY.
#define H2WR_LINKS_MAX 256  // (= GRDMA_H2_BATCH_MAX, include/grdma_amd.h)
struct h2wr_link {
  h2wr_dev* W;
};
#ifdef GRDMA_WAVE_EMU
#define H2WR_ENTRY(tab, l) ((tab)[l])
#else
#define H2WR_ENTRY(tab, l) (((const __attribute__((address_space(4))) h2wr_link*)(tab))[l])
#endif

#define H2WR_STAGE 1
__global__ __launch_bounds__(H2WR_THREADS) void k_h2_links_wr_queue(const h2wr_link* __restrict__ tab) {
  h2wr_dev* const W = H2WR_ENTRY(tab, blockIdx.x).W;
#include "grdma_h2_wr_stage.inc"
}
#undef H2WR_STAGE

#define H2WR_STAGE 2
__global__ __launch_bounds__(H2WR_THREADS) void k_h2_links_wr_commit(const h2wr_link* __restrict__ tab) {
  h2wr_dev* const W = H2WR_ENTRY(tab, blockIdx.x).W;
#include "grdma_h2_wr_stage.inc"
}
#undef H2WR_STAGE

}  // namespace
#endif  // GRDMA_H2_WR_H
