// HTTP/2 DATA framing (K6/K7) and deframing (K8/K9) on the device.
//
// TX  k_h2_frame_one (tables of more than 4096 messages: k_h2_frame_index + k_h2_frame_emit)
//                    builds, in HBM, the slice list chttp2 hands to
//                    grpc_endpoint_write for a batch of gRPC messages:
//                    5-byte message header (chttp2_transport.cc:1502-1510), 9-byte
//                    DATA frame headers (grpc_chttp2_encode_data, frame_data.cc:64-90),
//                    payload sub-slices by reference, with the inlined-slice merge
//                    rule of grpc_slice_buffer_add (slice_buffer.cc:136-171) and the
//                    split rule of move_first_no_ref (slice_buffer.cc:270-313).
//                    No payload byte is copied: K1 (k_copy) gathers straight from
//                    the message buffers.
//                    One wave per message (closed-form layout; sequential only around
//                    empty messages, whose inlined slices merge across message boundaries).
// RX  k_h2_deframe   the resumable frame-header state machine of
//                    grpc_chttp2_perform_read (parsing.cc:56-253) and the gRPC
//                    message deframer (frame_data.cc:92-276) over the slices an
//                    endpoint_read delivered.  Frame headers sit at data-dependent
//                    offsets (a linked list again); one wave stages the first 32
//                    bytes of the next 64 slices in registers so the automaton
//                    never waits on memory for a header that starts a slice -- the
//                    common case, because the ring preserves slice boundaries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "grdma_h2_kernels.h"
#include "grdma_h2_asm.h"
#include "grdma_h2_reply.h"
#include "grdma_h2_fc.h"
#include "grdma_h2_sw.h"
#include "grdma_h2_wr.h"
#include "grdma_h2_ctl.h"
#include "grdma_h2_hpack.h"
#include "grdma_h2_hpenc.h"
#include "grdma_h2_meta.h"
#include "grdma_h2_calls.h"
#include "grdma_h2_block.h"

// --------------------------------------------------------------------- host API
// Everything here runs on one non-blocking stream of its own and waits with
// hipStreamSynchronize: a device-wide synchronize would sit behind the resident latency
// engine until that idles out.  Scratch buffers and events are kept per parser / per process.
struct grdma_h2_parser {
  grdma_h2_parser_dev* d = nullptr;
  grdma_h2_stream_dev* d_tab = nullptr;
  grdma_slice_out* d_sl = nullptr;
  uint64_t sl_cap = 0;
  grdma_h2_event* d_ev = nullptr;
  uint64_t ev_cap = 0;
  grdma_h2_deframe_result* d_res = nullptr;
  grdma_h2_table_op* d_ops = nullptr;
  uint32_t ops_cap = 0;
  // the deframer over chunks (grdma_h2_kernels.h: grdma_h2_chunks): control block, private stream maps, event segments
  uint32_t slots = 0;
  int chunks_want = 0;                 // 0 = off
  grdma_h2_chunks* d_chunks = nullptr;
  grdma_h2_stream_dev* d_tabs = nullptr;
  grdma_h2_event* d_ev_tmp = nullptr;
  uint64_t ev_tmp_cap = 0;             // events the segments hold in total
  // the last deframing a pipe enqueued for this parser: the next one is ordered behind it (same stream, or this event)
  hipStream_t last_stream = nullptr;
  hipEvent_t last_deframed = nullptr;
  uint32_t asm_attached = 0;  // pipes that run an assembler of this parser behind their deframer
  // receive flow control (csrc/grdma_h2_fc.h): the parser's ledger, and the standalone deframings it may account --
  // their number and the event capacity of the last one (its events stay in d_ev / d_res until the next call)
  struct grdma_h2_fc* fc = nullptr;
  uint64_t standalone_calls = 0, standalone_ev_cap = 0;
  // send flow control (csrc/grdma_h2_sw.h): the parser's send windows, and what their intake reads of the last
  // standalone deframing beside its events -- the receive arena and the length of the slice table (d_sl)
  struct grdma_h2_sw* sw = nullptr;
  const uint8_t* standalone_arena = nullptr;
  uint64_t standalone_nsl = 0;
  // control replies (csrc/grdma_h2_ctl.h): the parser's control-reply writer; it reads what the send windows read
  struct grdma_h2_ctl* ctl = nullptr;
  // header blocks (csrc/grdma_h2_hpack.h): the parser's header decoder; it reads what the control-reply writer reads
  struct grdma_h2_hpack* hpack = nullptr;
};

// How many chunks a parser created without saying so cuts a long list into: GRDMA_H2_CHUNKS (default and at most 256, 0 or 1 = the
// sequential deframer only).
static int h2_chunks_default() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("GRDMA_H2_CHUNKS");
    v = e ? atoi(e) : H2_KMAX;
    if (v < 2) v = 0;
    if (v > H2_KMAX) v = H2_KMAX;
  }
  return v;
}

// (re)size the chunk buffers of a parser for calls that may produce ev_cap events
static bool h2_chunks_prepare(grdma_h2_parser* p, uint64_t ev_cap, hipStream_t st) {
  if (p->chunks_want < 2) return false;
  const uint64_t need = 4 * (ev_cap ? ev_cap : 1) + H2_KMAX * 64;
  if (p->d_chunks && p->ev_tmp_cap >= need) return true;
  if (!p->d_chunks) {
    if (hipMalloc((void**)&p->d_chunks, sizeof(grdma_h2_chunks)) != hipSuccess ||
        hipMalloc((void**)&p->d_tabs, sizeof(grdma_h2_stream_dev) * (size_t)H2_KMAX * p->slots) != hipSuccess)
      return false;
    if (hipMemsetAsync(p->d_chunks, 0, sizeof(grdma_h2_chunks), st) != hipSuccess) return false;
  }
  // The larger segment first, then the old one goes -- behind every deframing call that may still read it (another
  // pipe of this parser may run on another stream: the device is drained, this is a resize, not a hot path).  A
  // failure leaves the parser WITHOUT chunk buffers (capacity 0, chunks off) rather than with a control block that
  // points at freed memory.
  grdma_h2_event* bigger = nullptr;
  if (hipMalloc((void**)&bigger, sizeof(grdma_h2_event) * need) != hipSuccess) {
    (void)hipGetLastError();
    p->ev_tmp_cap = 0;
    p->chunks_want = 0;
    return false;
  }
  if (hipStreamSynchronize(st) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    hipFree(bigger);
    p->ev_tmp_cap = 0;
    p->chunks_want = 0;
    return false;
  }
  if (p->d_ev_tmp) hipFree(p->d_ev_tmp);
  p->d_ev_tmp = bigger;
  p->ev_tmp_cap = need;
  // the host-owned words of the control block (the counters stay)
  struct { grdma_h2_stream_dev* tabs; grdma_h2_event* ev_tmp; uint64_t ev_total; uint32_t slots, pad; } tail =
      {p->d_tabs, p->d_ev_tmp, need, p->slots, 0};
  static_assert(offsetof(grdma_h2_chunks, pad) + sizeof(uint32_t) - offsetof(grdma_h2_chunks, tabs) == sizeof(tail), "layout");
  const uint32_t want = (uint32_t)p->chunks_want;
  const bool ok = hipMemcpyAsync(reinterpret_cast<uint8_t*>(p->d_chunks) + offsetof(grdma_h2_chunks, tabs), &tail, sizeof(tail),
                                 hipMemcpyHostToDevice, st) == hipSuccess &&
                  hipMemcpyAsync(reinterpret_cast<uint8_t*>(p->d_chunks) + offsetof(grdma_h2_chunks, want), &want, sizeof(want),
                                 hipMemcpyHostToDevice, st) == hipSuccess &&
                  hipStreamSynchronize(st) == hipSuccess;
  if (!ok) {  // (the control block may not know the new segment: no chunked deframing with it)
    p->ev_tmp_cap = 0;
    p->chunks_want = 0;
  }
  return ok;
}

// --------------------------------------------------------------------- stages
// A stage is one kernel chain as a list of grdma_job_hook records (csrc/grdma_dev.h: the kernel, its launch shape, its
// parameters).  A chain is written down ONCE, by one of the builders below, and the list is used both ways: as kernel
// nodes of a streaming job's graph (grdma_job_set_hooks) and launched on a stream (h2_launch).  The standalone calls,
// the batch calls (csrc/grdma_h2_host_calls.inc) and both kinds of pipe (csrc/grdma_h2_host_pipe.inc) take their kernels
// from here and nowhere else.
typedef std::vector<grdma_job_hook> h2_stage;

static uint64_t h2_slot(const void* p) { return (uint64_t)(uintptr_t)p; }
static uint64_t h2_slot(uint64_t v) { return v; }
// one record: the arguments are held against the kernel's parameter list (their number, and each converts to its type)
template <typename... P, typename... A>
static grdma_job_hook h2_rec(void (*k)(P...), uint32_t grid, uint32_t threads, A... a) {
  static_assert(sizeof...(P) == sizeof...(A) && sizeof...(P) <= GRDMA_JOB_HOOK_ARGS, "one argument per kernel parameter");
  return grdma_job_hook{(const void*)k, grid, threads, {h2_slot(static_cast<P>(a))...}};
}

// n records launched on st, in order (the runtime reads as many parameter slots as the kernel has); the first launch
// the runtime refuses ends it
static hipError_t h2_launch(const grdma_job_hook* recs, size_t n, hipStream_t st) {
  for (size_t i = 0; i < n; i++) {
    void* args[GRDMA_JOB_HOOK_ARGS];
    for (uint32_t a = 0; a < GRDMA_JOB_HOOK_ARGS; a++) args[a] = const_cast<uint64_t*>(&recs[i].args[a]);
    const hipError_t e = hipLaunchKernel(recs[i].fn, dim3(recs[i].grid), dim3(recs[i].threads), args, 0, st);
    if (e != hipSuccess) {
      (void)hipGetLastError();  // (reported here: no later call finds it)
      return e;
    }
  }
  return hipSuccess;
}
static hipError_t h2_launch(const h2_stage& s, hipStream_t st) { return h2_launch(s.data(), s.size(), st); }

// The framing of one message table: one launch in which every workgroup sums what lies in front of its messages itself;
// above H2_FRAME_ONE_MAX messages sizes and positions first, then one wave per message (grdma_h2_kernels.h).
static h2_stage h2_stage_frame(const grdma_h2_msg_dev* d_msgs, uint64_t n, uint32_t max_frame, grdma_sge* out, uint64_t cap,
                               uint8_t* hdr, uint64_t hdr_cap, grdma_h2_msg_pos* d_pos, grdma_h2_frame_result* d_res) {
  const uint64_t per = H2_EMIT_THREADS / 64;
  const uint32_t grid = (uint32_t)((n + per - 1) / per);
  if (n <= H2_FRAME_ONE_MAX)
    return {h2_rec(k_h2_frame_one, grid, H2_EMIT_THREADS, d_msgs, n, max_frame, out, cap, hdr, hdr_cap, d_res)};
  return {h2_rec(k_h2_frame_index, 1, 256, d_msgs, n, max_frame, cap, hdr_cap, d_pos, d_res),
          h2_rec(k_h2_frame_emit, grid, H2_EMIT_THREADS, d_msgs, n, max_frame, out, cap, hdr, hdr_cap, d_pos)};
}
// ... of the message tables of many links (grid: the workgroups of all links, grdma_h2_link_frame::wg0)
static h2_stage h2_stage_frame_links(const grdma_h2_link_frame* d_tab, uint32_t n, uint32_t grid) {
  return {h2_rec(k_h2_frame_links, grid, H2_EMIT_THREADS, d_tab, n)};
}

// The deframing of one list of delivered slices: over chunks when the parser has the buffers (chunked: h2_chunks_prepare
// said so) and the list is long enough -- plan, the chunks side by side, then the merge, or the sequential deframer over
// the whole list when the chain did not hold -- else the sequential deframer alone.
static h2_stage h2_stage_deframe(const grdma_h2_parser* p, const uint8_t* arena, const grdma_slice_out* d_slices, uint64_t n,
                                 grdma_h2_event* d_ev, uint64_t ev_cap, grdma_h2_deframe_result* d_res, bool chunked) {
  if (!chunked || n < H2_CHUNK_MIN_SLICES)
    return {h2_rec(k_h2_deframe, 1, H2_DEFRAME_THREADS, p->d, arena, d_slices, n, d_ev, ev_cap, d_res)};
  return {h2_rec(k_h2_deframe_chunks, (uint32_t)p->chunks_want, H2_DEFRAME_THREADS, p->d, p->d_chunks, arena, d_slices, n),
          h2_rec(k_h2_merge_or_deframe, H2_MERGE_GRID, H2_DEFRAME_THREADS, p->d, p->d_chunks, arena, d_slices, n, d_ev, ev_cap,
                 d_res)};
}
// ... of the lists of n links, one workgroup each
static h2_stage h2_stage_deframe_links(const grdma_h2_link_deframe* d_tab, uint32_t n) {
  return {h2_rec(k_h2_deframe_links, n, H2_DEFRAME_THREADS, d_tab)};
}

// The assembly of one call behind its deframing (csrc/grdma_h2_asm.h): the plan, records [0, 5), then the copy.
static h2_stage h2_stage_asm(h2a_dev* d, const h2a_call* d_call) {
  return {h2_rec(k_h2_asm_tiles, H2A_GRID, H2A_THREADS, d, d_call),
          h2_rec(k_h2_asm_carry, 1, H2A_ONE_THREADS, d, d_call),
          h2_rec(k_h2_asm_begin, H2A_GRID, H2A_THREADS, d, d_call),
          h2_rec(k_h2_asm_bytes, H2A_GRID, H2A_THREADS, d, d_call),
          h2_rec(k_h2_asm_finish, 1, H2A_ONE_THREADS, d, d_call),
          h2_rec(k_h2_asm_copy, H2A_GRID, H2A_THREADS, d, d_call)};
}
// ... of n links in the same six launches: the plan's one-workgroup stages of the links run side by side
static_assert(H2A_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the assembler's link table is the batch's");
static h2_stage h2_stage_asm_links(const h2a_link* d_tab, uint32_t n) {
  return {h2_rec(k_h2_asm_tiles_links, n * H2A_LINK_GRID, H2A_THREADS, d_tab, n),
          h2_rec(k_h2_asm_carry_links, n, H2A_ONE_THREADS, d_tab),
          h2_rec(k_h2_asm_begin_links, n * H2A_LINK_GRID, H2A_THREADS, d_tab, n),
          h2_rec(k_h2_asm_bytes_links, n * H2A_LINK_GRID, H2A_THREADS, d_tab, n),
          h2_rec(k_h2_asm_finish_links, n, H2A_ONE_THREADS, d_tab),
          h2_rec(k_h2_asm_copy_links, H2A_GRID, H2A_THREADS, d_tab, n)};
}
static const size_t H2_ASM_PLAN = 5;  // records of an assembler stage in front of its copy (timed apart by the standalone calls)

// The reply framer of one transport (csrc/grdma_h2_reply.h): plan, then emit -- in front of a job a linear chain.
static h2_stage h2_stage_reply(h2r_dev* d) {
  return {h2_rec(k_h2_reply_plan, 1, PLAN_THREADS, d), h2_rec(k_h2_reply_emit, H2R_GRID, H2_EMIT_THREADS, d)};
}
// ... of n links in the same two launches
static_assert(H2R_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the reply's link table is the batch's");
static h2_stage h2_stage_reply_links(const h2r_link* d_tab, uint32_t n) {
  return {h2_rec(k_h2_reply_plan_links, n, PLAN_THREADS, d_tab), h2_rec(k_h2_reply_emit_links, H2R_GRID, H2_EMIT_THREADS, d_tab, n)};
}

// The window ledger of one call behind its deframing (csrc/grdma_h2_fc.h): it reads the events only, so it may stand in
// front of, behind or beside an assembler's stage.
static h2_stage h2_stage_fc(h2fc_dev* d, const h2fc_call* d_call) {
  return {h2_rec(k_h2_fc_clear, H2FC_GRID, H2FC_THREADS, d, d_call), h2_rec(k_h2_fc_keys, H2FC_GRID, H2FC_THREADS, d, d_call),
          h2_rec(k_h2_fc_sums, H2FC_GRID, H2FC_THREADS, d, d_call), h2_rec(k_h2_fc_finish, 1, H2FC_ONE_THREADS, d, d_call),
          h2_rec(k_h2_fc_emit, H2FC_GRID, H2FC_THREADS, d)};
}
// ... of n links in the same five launches: every link a share of the grid, the one-workgroup stage side by side
static_assert(H2FC_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the ledger's link table is the batch's");
static h2_stage h2_stage_fc_links(const h2fc_link* d_tab, uint32_t n) {
  return {h2_rec(k_h2_links_fc_clear, n * H2FC_LINK_GRID, H2FC_THREADS, d_tab, n),
          h2_rec(k_h2_links_fc_keys, n * H2FC_LINK_GRID, H2FC_THREADS, d_tab, n),
          h2_rec(k_h2_links_fc_sums, n * H2FC_LINK_GRID, H2FC_THREADS, d_tab, n),
          h2_rec(k_h2_links_fc_finish, n, H2FC_ONE_THREADS, d_tab),
          h2_rec(k_h2_links_fc_emit, n * H2FC_LINK_GRID, H2FC_THREADS, d_tab, n)};
}

// The intake of the send windows behind a deframing (csrc/grdma_h2_sw.h): it reads the events, the slice table and the
// receive arena; and their framer: plan, then emit, as the reply's.
static h2_stage h2_stage_sw_intake(h2sw_dev* d, const h2sw_call* d_call) {
  return {h2_rec(k_h2_sw_clear, H2SW_GRID, H2SW_THREADS, d), h2_rec(k_h2_sw_take, H2SW_GRID, H2SW_THREADS, d, d_call),
          h2_rec(k_h2_sw_finish, 1, H2SW_THREADS, d, d_call)};
}
static h2_stage h2_stage_sw_frame(h2sw_dev* d) {
  return {h2_rec(k_h2_sw_plan, 1, H2SW_PLAN_THREADS, d), h2_rec(k_h2_sw_emit, H2SW_GRID, H2_EMIT_THREADS, d)};
}
// ... of n links in the same three and two launches: every link a share of the grid, the one-workgroup stages side by side
static_assert(H2SW_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the send windows' link table is the batch's");
static h2_stage h2_stage_sw_intake_links(const h2sw_link* d_tab, uint32_t n) {
  return {h2_rec(k_h2_links_sw_clear, n * H2SW_LINK_GRID, H2SW_THREADS, d_tab, n),
          h2_rec(k_h2_links_sw_take, n * H2SW_LINK_GRID, H2SW_THREADS, d_tab, n),
          h2_rec(k_h2_links_sw_finish, n, H2SW_THREADS, d_tab)};
}
static h2_stage h2_stage_sw_frame_links(const h2sw_link* d_tab, uint32_t n) {
  return {h2_rec(k_h2_links_sw_plan, n, H2SW_PLAN_THREADS, d_tab), h2_rec(k_h2_links_sw_emit, H2SW_GRID, H2_EMIT_THREADS, d_tab, n)};
}

// The reply under the send windows (csrc/grdma_h2_wr.h): the queue stage builds the plan's table in device memory, the
// send windows' framer runs unchanged over it, the commit keeps what the windows cut off.
static h2_stage h2_stage_wr_frame(h2wr_dev* d, h2sw_dev* sw) {
  return {h2_rec(k_h2_wr_queue, 1, H2WR_THREADS, d), h2_rec(k_h2_sw_plan, 1, H2SW_PLAN_THREADS, sw),
          h2_rec(k_h2_sw_emit, H2SW_GRID, H2_EMIT_THREADS, sw), h2_rec(k_h2_wr_commit, 1, H2WR_THREADS, d)};
}
// ... of n links in the same four launches
static_assert(H2WR_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the windowed reply's link table is the batch's");
static h2_stage h2_stage_wr_frame_links(const h2wr_link* d_tab, const h2sw_link* d_sw_tab, uint32_t n) {
  return {h2_rec(k_h2_links_wr_queue, n, H2WR_THREADS, d_tab), h2_rec(k_h2_links_sw_plan, n, H2SW_PLAN_THREADS, d_sw_tab),
          h2_rec(k_h2_links_sw_emit, H2SW_GRID, H2_EMIT_THREADS, d_sw_tab, n), h2_rec(k_h2_links_wr_commit, n, H2WR_THREADS, d_tab)};
}

// The control-reply writer behind a deframing (csrc/grdma_h2_ctl.h): it reads the events, the slice table and the
// receive arena, as the intake of the send windows does.
static h2_stage h2_stage_ctl(h2ctl_dev* d, const h2ctl_call* d_call) {
  return {h2_rec(k_h2_ctl_last, H2CTL_GRID, H2CTL_THREADS, d, d_call), h2_rec(k_h2_ctl_mark, H2CTL_GRID, H2CTL_THREADS, d, d_call),
          h2_rec(k_h2_ctl_scan, 1, H2CTL_THREADS, d, d_call), h2_rec(k_h2_ctl_emit, H2CTL_GRID, H2CTL_THREADS, d, d_call)};
}
// ... of n links in the same four launches: every link a share of the grid, the scans side by side
static_assert(H2CTL_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the control-reply writer's link table is the batch's");
static_assert(H2CTL_GRID <= H2CTL_GRID_MAX && H2CTL_LINK_GRID <= H2CTL_GRID_MAX && H2CTL_GRID_MAX <= H2CTL_THREADS,
              "the scan reads one workgroup's counts per thread");
static h2_stage h2_stage_ctl_links(const h2ctl_link* d_tab, uint32_t n) {
  return {h2_rec(k_h2_links_ctl_last, n * H2CTL_LINK_GRID, H2CTL_THREADS, d_tab, n),
          h2_rec(k_h2_links_ctl_mark, n * H2CTL_LINK_GRID, H2CTL_THREADS, d_tab, n),
          h2_rec(k_h2_links_ctl_scan, n, H2CTL_THREADS, d_tab),
          h2_rec(k_h2_links_ctl_emit, n * H2CTL_LINK_GRID, H2CTL_THREADS, d_tab, n)};
}

// The header decoder behind a deframing (csrc/grdma_h2_hpack.h): the gather, whose totals the host sizes the scratch of the
// other stages by, and those stages.
static h2_stage h2_stage_hpack_gather(h2hp_dev* d, const h2hp_call* d_call) {
  return {h2_rec(k_h2_hpack_gather, 1, H2HP_THREADS, d, d_call)};
}
static h2_stage h2_stage_hpack_decode(h2hp_dev* d, const h2hp_call* d_call) {
  return {h2_rec(k_h2_hpack_copy, H2HP_GRID, H2HP_THREADS, d, d_call), h2_rec(k_h2_hpack_split, H2HP_GRID, H2HP_THREADS, d, d_call),
          h2_rec(k_h2_hpack_walk, 1, H2HP_THREADS, d, d_call), h2_rec(k_h2_hpack_emit, H2HP_GRID, H2HP_THREADS, d, d_call),
          h2_rec(k_h2_hpack_commit, H2HP_GRID, H2HP_THREADS, d, d_call)};
}
static h2_stage h2_stage_hpack_resize(h2hp_dev* d) { return {h2_rec(k_h2_hpack_resize, 1, 64, d)}; }
// ... of n links in the same six launches: the gathers and the walks side by side, every link a share of the grid stages
static_assert(H2HP_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the header decoder's link table is the batch's");
static h2_stage h2_stage_hpack_links_gather(const h2hp_link* d_tab, uint32_t n) {
  return {h2_rec(k_h2_links_hpack_gather, n, H2HP_THREADS, d_tab, n)};
}
static h2_stage h2_stage_hpack_links_decode(const h2hp_link* d_tab, uint32_t n) {
  return {h2_rec(k_h2_links_hpack_copy, n * H2HP_LINK_GRID, H2HP_THREADS, d_tab, n),
          h2_rec(k_h2_links_hpack_split, n * H2HP_LINK_GRID, H2HP_THREADS, d_tab, n),
          h2_rec(k_h2_links_hpack_walk, n, H2HP_THREADS, d_tab, n),
          h2_rec(k_h2_links_hpack_emit, n * H2HP_LINK_GRID, H2HP_THREADS, d_tab, n),
          h2_rec(k_h2_links_hpack_commit, n * H2HP_LINK_GRID, H2HP_THREADS, d_tab, n)};
}

// The header encoder (csrc/grdma_h2_hpenc.h): it belongs to no parser.  Three sections, timed apart: scan, walk, emit and
// commit.
static h2_stage h2_stage_hpenc(h2he_dev* d) {
  return {h2_rec(k_h2_hpenc_scan, H2HE_GRID, H2HE_THREADS, d), h2_rec(k_h2_hpenc_walk, 1, H2HE_THREADS, d),
          h2_rec(k_h2_hpenc_emit, H2HE_GRID, H2HE_THREADS, d), h2_rec(k_h2_hpenc_commit, H2HE_GRID, H2HE_THREADS, d)};
}
// ... of n links in the same four launches and the same three sections: the walks side by side, every link a share of
// the grid stages
static_assert(H2HE_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the header encoder's link table is the batch's");
static h2_stage h2_stage_hpenc_links(const h2he_link* d_tab, uint32_t n) {
  return {h2_rec(k_h2_links_hpenc_scan, n * H2HE_LINK_GRID, H2HE_THREADS, d_tab, n),
          h2_rec(k_h2_links_hpenc_walk, n, H2HE_THREADS, d_tab, n),
          h2_rec(k_h2_links_hpenc_emit, n * H2HE_LINK_GRID, H2HE_THREADS, d_tab, n),
          h2_rec(k_h2_links_hpenc_commit, n * H2HE_LINK_GRID, H2HE_THREADS, d_tab, n)};
}

// The metadata reader (csrc/grdma_h2_meta.h): it belongs to no parser.  One section.
static h2_stage h2_stage_meta(h2m_dev* d) {
  return {h2_rec(k_h2_meta_fields, H2M_GRID, H2M_THREADS, d), h2_rec(k_h2_meta_blocks, H2M_GRID, H2M_BLK_THREADS, d),
          h2_rec(k_h2_meta_emit, H2M_GRID, H2M_THREADS, d)};
}
// ... of n links in the same three launches: ONE reader (its constants, its counters), every link a share of the grid
static_assert(H2M_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the metadata reader's link table is the batch's");
static h2_stage h2_stage_meta_links(h2m_dev* d, const h2m_link* d_tab, uint32_t n) {
  return {h2_rec(k_h2_links_meta_fields, n * H2M_LINK_GRID, H2M_THREADS, d, d_tab, n),
          h2_rec(k_h2_links_meta_blocks, n * H2M_LINK_GRID, H2M_BLK_THREADS, d, d_tab, n),
          h2_rec(k_h2_links_meta_emit, n * H2M_LINK_GRID, H2M_THREADS, d, d_tab, n)};
}

// The call table (csrc/grdma_h2_calls.h): it belongs to no parser.  One section, eight launches whatever the counts.
static h2_stage h2_stage_calls(h2c_dev* d) {
  return {h2_rec(k_h2_calls_clear, H2C_GRID, H2C_THREADS, d),  h2_rec(k_h2_calls_claim, H2C_GRID, H2C_THREADS, d),
          h2_rec(k_h2_calls_wins, H2C_GRID, H2C_THREADS, d),   h2_rec(k_h2_calls_insert, H2C_GRID, H2C_THREADS, d),
          h2_rec(k_h2_calls_msgs, H2C_GRID, H2C_THREADS, d),   h2_rec(k_h2_calls_cols, H2C_GRID, H2C_THREADS, d),
          h2_rec(k_h2_calls_finish, 1, H2C_THREADS, d),        h2_rec(k_h2_calls_emit, H2C_GRID, H2C_THREADS, d)};
}
// ... of n links' tables in the same eight launches: every link a share of the grid stages, the finishes side by side
static_assert(H2C_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the call table's link table is the batch's");
static h2_stage h2_stage_calls_links(const h2c_link* d_tab, uint32_t n) {
  const uint32_t grid = n * H2C_LINK_GRID;
  return {h2_rec(k_h2_links_calls_clear, grid, H2C_THREADS, d_tab, n),  h2_rec(k_h2_links_calls_claim, grid, H2C_THREADS, d_tab, n),
          h2_rec(k_h2_links_calls_wins, grid, H2C_THREADS, d_tab, n),   h2_rec(k_h2_links_calls_insert, grid, H2C_THREADS, d_tab, n),
          h2_rec(k_h2_links_calls_msgs, grid, H2C_THREADS, d_tab, n),   h2_rec(k_h2_links_calls_cols, grid, H2C_THREADS, d_tab, n),
          h2_rec(k_h2_links_calls_finish, n, H2C_THREADS, d_tab, n),    h2_rec(k_h2_links_calls_emit, grid, H2C_THREADS, d_tab, n)};
}

// st goes behind the parser's last deframing by a pipe (the parser state is handed from one deframing to the next),
// unless that one was enqueued on st itself.  (Only pipe steps leave last_deframed, on a job's or a deframe stream: for
// the standalone calls, on the stream of their own, the exception never holds and they always wait.)
static bool h2_wait_parser(hipStream_t st, const grdma_h2_parser* p) {
  return !p->last_deframed || p->last_stream == st || hipStreamWaitEvent(st, p->last_deframed, 0) == hipSuccess;
}

// a host message table in the device's form: into tab, or as a table of its own
static void h2_msg_rows(const grdma_h2_msg* msgs, uint64_t n, grdma_h2_msg_dev* tab) {
  for (uint64_t i = 0; i < n; i++) {
    tab[i].payload = static_cast<const uint8_t*>(msgs[i].payload);
    tab[i].len = msgs[i].len;
    tab[i].stream_id = msgs[i].stream_id;
    tab[i].flags = msgs[i].flags;
  }
}
static std::vector<grdma_h2_msg_dev> h2_msg_table(const grdma_h2_msg* msgs, uint64_t n) {
  std::vector<grdma_h2_msg_dev> tab(n);
  h2_msg_rows(msgs, n, tab.data());
  return tab;
}
// ... uploaded to a device table of its own (a pipe's: the caller frees it)
static bool h2_upload_msgs(const grdma_h2_msg* msgs, uint64_t n, grdma_h2_msg_dev** d_msgs) {
  const std::vector<grdma_h2_msg_dev> tab = h2_msg_table(msgs, n);
  return hipMalloc((void**)d_msgs, sizeof(grdma_h2_msg_dev) * n) == hipSuccess &&
         hipMemcpy(*d_msgs, tab.data(), sizeof(grdma_h2_msg_dev) * n, hipMemcpyHostToDevice) == hipSuccess;
}

// 64 frames per bulk step (GRDMA_H2_BULK_PAIRS): on unless GRDMA_H2_NO_BULK_PAIRS or GRDMA_H2_BULK_PAIRS=0 says otherwise
static int h2_bulk_pairs_default() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("GRDMA_H2_BULK_PAIRS");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v;
}
// What a parser created without either flag does: the boundary step is on unless the environment
// says GRDMA_H2_BOUNDARY_STEP=0.
static int h2_boundary_default() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("GRDMA_H2_BOUNDARY_STEP");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v;
}

namespace {
// The one stream of the standalone and batch calls (csrc/grdma_h2_host_calls.inc) and the stamps of their timed
// sections: a call of k sections records stamp[0 .. k] (h2_call_run).  The calls run one at a time on this stream, so
// one set serves them all; the pipes time their stages with events of their own.
struct h2_host_ctx {
  hipStream_t stream = nullptr;
  hipEvent_t stamp[4] = {nullptr, nullptr, nullptr, nullptr};
};
h2_host_ctx* h2_ctx() {
  static h2_host_ctx c;
  if (!c.stream) {
    if (hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
    for (hipEvent_t& e : c.stamp)
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
  }
  return &c;
}
template <typename T>
bool h2_grow(T** buf, uint64_t* cap, uint64_t need) {
  if (need <= *cap && *buf) return true;
  if (*buf) hipFree(*buf);
  *buf = nullptr;
  uint64_t n = *cap ? *cap : 64;
  while (n < need) n *= 2;
  if (hipMalloc((void**)buf, sizeof(T) * n) != hipSuccess) { *cap = 0; return false; }
  *cap = n;
  return true;
}
}  // namespace

extern "C" {

const char* grdma_last_error(void);
int grdma_fail_msg(int code, const char* msg);  // (csrc/grdma_pair.hip: sets grdma_last_error, returns -code)

#include "grdma_h2_host_calls.inc"
#include "grdma_h2_host_pipe.inc"

}  // extern "C"
