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
#include <vector>

#include "grdma_h2_kernels.h"
#include "grdma_h2_asm.h"
#include "grdma_h2_reply.h"
#include "grdma_h2_fc.h"

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
// the batch calls and both kinds of pipe (csrc/grdma_h2_host_pipe.inc) take their kernels from here and nowhere else.
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

// st goes behind the parser's last deframing by a pipe (the parser state is handed from one deframing to the next),
// unless that one was enqueued on st itself.  (Only pipe steps leave last_deframed, on a job's or a deframe stream: for
// the standalone calls, on the stream of their own, the exception never holds and they always wait.)
static bool h2_wait_parser(hipStream_t st, const grdma_h2_parser* p) {
  return !p->last_deframed || p->last_stream == st || hipStreamWaitEvent(st, p->last_deframed, 0) == hipSuccess;
}

// a host message table in the device's form
static std::vector<grdma_h2_msg_dev> h2_msg_table(const grdma_h2_msg* msgs, uint64_t n) {
  std::vector<grdma_h2_msg_dev> tab(n);
  for (uint64_t i = 0; i < n; i++) {
    tab[i].payload = static_cast<const uint8_t*>(msgs[i].payload);
    tab[i].len = msgs[i].len;
    tab[i].stream_id = msgs[i].stream_id;
    tab[i].flags = msgs[i].flags;
  }
  return tab;
}
// ... uploaded to a device table of its own (a pipe's: the caller frees it)
static bool h2_upload_msgs(const grdma_h2_msg* msgs, uint64_t n, grdma_h2_msg_dev** d_msgs) {
  const std::vector<grdma_h2_msg_dev> tab = h2_msg_table(msgs, n);
  return hipMalloc((void**)d_msgs, sizeof(grdma_h2_msg_dev) * n) == hipSuccess &&
         hipMemcpy(*d_msgs, tab.data(), sizeof(grdma_h2_msg_dev) * n, hipMemcpyHostToDevice) == hipSuccess;
}

static double g_h2_last_kernel_us = 0;
static uint64_t g_h2_last_boundary_steps = 0;
static uint64_t g_h2_last_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

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
struct h2_host_ctx {
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};
h2_host_ctx* h2_ctx() {
  static h2_host_ctx c;
  if (!c.stream) {
    if (hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
    if (hipEventCreate(&c.e0) != hipSuccess || hipEventCreate(&c.e1) != hipSuccess) return nullptr;
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
// duration of the framing / deframing kernel of the last call (HIP events), microseconds
double grdma_h2_last_kernel_us(void) { return g_h2_last_kernel_us; }
// message starts the last grdma_h2_deframe call took through the boundary step
uint64_t grdma_h2_last_boundary_steps(void) { return g_h2_last_boundary_steps; }
// counters of the last grdma_h2_deframe call: {bulk steps, frames parsed in bulk steps, boundary steps,
// then device-clock ticks: waiting for staged windows, in bulk steps, in boundary steps, in the
// byte-wise path, total}
void grdma_h2_last_deframe_stats(uint64_t out[8]) {
  for (int i = 0; i < 8; i++) out[i] = g_h2_last_stats[i];
}

int64_t grdma_h2_frame_messages(const grdma_h2_msg* msgs, uint64_t n, uint32_t max_frame,
                                grdma_slice* d_slices_out, uint64_t slices_cap,
                                void* d_hdr_arena, uint64_t hdr_cap, uint64_t* wire_bytes) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!msgs || !n || !d_slices_out || !d_hdr_arena || max_frame == 0 || max_frame >= (1u << 24))
    return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  for (uint64_t i = 0; i < n; i++)
    if (msgs[i].len >= (1ull << 32)) return -GRDMA_ERR_INVALID;  // 32-bit message length field
  const std::vector<grdma_h2_msg_dev> tmp = h2_msg_table(msgs, n);
  static grdma_h2_msg_dev* d_msgs = nullptr;
  static uint64_t msgs_cap = 0;
  static grdma_h2_frame_result* d_res = nullptr;
  static grdma_h2_msg_pos* d_pos = nullptr;
  static uint64_t pos_cap = 0;
  grdma_h2_frame_result h_res;
  if (!h2_grow(&d_msgs, &msgs_cap, n) || !h2_grow(&d_pos, &pos_cap, n)) return -GRDMA_ERR_HIP;
  if (!d_res && hipMalloc((void**)&d_res, sizeof(grdma_h2_frame_result)) != hipSuccess) return -GRDMA_ERR_HIP;
  hipStream_t st = hc->stream;
  if (hipMemcpyAsync(d_msgs, tmp.data(), sizeof(grdma_h2_msg_dev) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(d_res, 0, sizeof(grdma_h2_frame_result), st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  hipEventRecord(hc->e0, st);
  const hipError_t launched = h2_launch(h2_stage_frame(d_msgs, n, max_frame, reinterpret_cast<grdma_sge*>(d_slices_out), slices_cap,
                                                       static_cast<uint8_t*>(d_hdr_arena), hdr_cap, d_pos, d_res), st);
  hipEventRecord(hc->e1, st);
  if (launched != hipSuccess || hipMemcpyAsync(&h_res, d_res, sizeof(h_res), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  float ms = 0;
  if (hipEventElapsedTime(&ms, hc->e0, hc->e1) == hipSuccess) g_h2_last_kernel_us = 1e3 * ms;
  if (h_res.overflow) return -GRDMA_ERR_CAPACITY;
  if (wire_bytes) *wire_bytes = h_res.wire_bytes;
  return (int64_t)h_res.nslices;
}

grdma_h2_parser* grdma_h2_parser_create_ex(int flags, uint32_t max_frame_size,
                                           uint32_t max_concurrent_streams, uint32_t table_slots) {
  if (grdma_device_count() <= 0) return nullptr;
  if (table_slots == 0) table_slots = 4096;
  if (table_slots < 16 || (table_slots & (table_slots - 1)) != 0) return nullptr;
  grdma_h2_parser* p = new grdma_h2_parser();
  grdma_h2_parser_dev init;
  memset(&init, 0, sizeof(init));
  init.is_server = (flags & GRDMA_H2_SERVER) ? 1 : 0;
  init.is_first_frame = (flags & GRDMA_H2_FIRST_FRAME) ? 1 : 0;  // chttp2_transport.cc: t->is_first_frame
  init.state = init.is_server ? 0 : 24;        // a server starts at GRPC_DTS_CLIENT_PREFIX_0
  init.max_frame_size = max_frame_size;        // http2_settings.cc:56 default 16384
  init.max_concurrent = max_concurrent_streams;  // http2_settings.cc:46 default 0xffffffff
  init.tab_mask = table_slots - 1;
  init.boundary_step = (flags & GRDMA_H2_BOUNDARY_STEP) ? 1 : (flags & GRDMA_H2_NO_BOUNDARY_STEP) ? 0 : h2_boundary_default();
  init.bulk_pairs = (flags & GRDMA_H2_BULK_PAIRS) ? 1 : (flags & GRDMA_H2_NO_BULK_PAIRS) ? 0 : h2_bulk_pairs_default();
  init.ticks = (flags & GRDMA_H2_TICKS) ? 1 : 0;
  p->slots = table_slots;
  p->chunks_want = (flags & GRDMA_H2_NO_CHUNKS) ? 0 : h2_chunks_default();
  if (hipMalloc((void**)&p->d, sizeof(init)) != hipSuccess ||
      hipMalloc((void**)&p->d_tab, sizeof(grdma_h2_stream_dev) * table_slots) != hipSuccess ||
      hipMalloc((void**)&p->d_res, sizeof(grdma_h2_deframe_result)) != hipSuccess ||
      hipMemset(p->d_tab, 0, sizeof(grdma_h2_stream_dev) * table_slots) != hipSuccess) {
    grdma_h2_parser_destroy(p);
    return nullptr;
  }
  init.tab = p->d_tab;
  if (hipMemcpy(p->d, &init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) {
    grdma_h2_parser_destroy(p);
    return nullptr;
  }
  return p;
}

grdma_h2_parser* grdma_h2_parser_create(int expect_client_prefix, uint32_t max_frame_size) {
  return grdma_h2_parser_create_ex(expect_client_prefix ? (GRDMA_H2_SERVER | GRDMA_H2_FIRST_FRAME) : 0,
                                   max_frame_size, 0xffffffffu, 0);
}

static void h2_fc_parser_gone(struct grdma_h2_fc* f);
void grdma_h2_parser_destroy(grdma_h2_parser* p) {
  if (!p) return;
  if (p->fc) h2_fc_parser_gone(p->fc);  // (the ledger outlives its parser as a husk: every call on it is refused)
  hipFree(p->d);
  hipFree(p->d_tab);
  hipFree(p->d_sl);
  hipFree(p->d_ev);
  hipFree(p->d_res);
  hipFree(p->d_ops);
  hipFree(p->d_chunks);
  hipFree(p->d_tabs);
  hipFree(p->d_ev_tmp);
  delete p;
}

static int h2_table_ops(grdma_h2_parser* p, uint32_t op, const uint32_t* ids, uint32_t n) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || (!ids && n)) return -GRDMA_ERR_INVALID;
  if (n == 0) return 0;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  uint64_t cap = p->ops_cap;
  if (!h2_grow(&p->d_ops, &cap, n)) return -GRDMA_ERR_HIP;
  p->ops_cap = (uint32_t)cap;
  std::vector<grdma_h2_table_op> h(n);
  for (uint32_t i = 0; i < n; i++) h[i] = {op, ids[i], 0, 0};
  hipStream_t st = hc->stream;
  if (hipMemcpyAsync(p->d_ops, h.data(), sizeof(grdma_h2_table_op) * n, hipMemcpyHostToDevice, st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  hipLaunchKernelGGL(k_h2_table_ops, dim3(1), dim3(1), 0, st, p->d, p->d_ops, n);
  if (hipMemcpyAsync(h.data(), p->d_ops, sizeof(grdma_h2_table_op) * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  int failed = 0;
  for (uint32_t i = 0; i < n; i++) failed += h[i].rc != 0;
  return failed;
}

int grdma_h2_parser_open_streams(grdma_h2_parser* p, const uint32_t* ids, uint32_t n) {
  return h2_table_ops(p, 1, ids, n);
}
int grdma_h2_parser_close_writes(grdma_h2_parser* p, const uint32_t* ids, uint32_t n) {
  return h2_table_ops(p, 2, ids, n);
}
// {calls the chunked deframer planned, calls whose chunks verified and were merged} since the parser was created
int grdma_h2_parser_chunk_stats(grdma_h2_parser* p, uint64_t out[2]) {
  if (!p || !out) return -GRDMA_ERR_INVALID;
  out[0] = out[1] = 0;
  if (!p->d_chunks) return 0;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  uint64_t v[2];
  if (hipMemcpyAsync(v, reinterpret_cast<uint8_t*>(p->d_chunks) + offsetof(grdma_h2_chunks, n_planned), sizeof(v),
                     hipMemcpyDeviceToHost, hc->stream) != hipSuccess ||
      hipStreamSynchronize(hc->stream) != hipSuccess)
    return -GRDMA_ERR_HIP;
  out[0] = v[0];
  out[1] = v[1];
  return 0;
}
// profiling aid: the phase stamps of the last chunked call, (H2_KMAX + 1) rows of 8 (csrc/grdma_h2_kernels.h)
int grdma_h2_parser_chunk_dbg(grdma_h2_parser* p, uint64_t* out, uint64_t cap_words) {
  if (!p || !out || !p->d_chunks) return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  const uint64_t words = std::min<uint64_t>(cap_words, (H2_KMAX + 1) * 8);
  if (hipMemcpyAsync(out, reinterpret_cast<uint8_t*>(p->d_chunks) + offsetof(grdma_h2_chunks, dbg), words * 8,
                     hipMemcpyDeviceToHost, hc->stream) != hipSuccess ||
      hipStreamSynchronize(hc->stream) != hipSuccess)
    return -GRDMA_ERR_HIP;
  return (int)words;
}
int64_t grdma_h2_parser_live_streams(grdma_h2_parser* p) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p) return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  grdma_h2_parser_dev h;
  if (hipMemcpyAsync(&h, p->d, sizeof(h), hipMemcpyDeviceToHost, hc->stream) != hipSuccess ||
      hipStreamSynchronize(hc->stream) != hipSuccess)
    return -GRDMA_ERR_HIP;
  return (int64_t)h.live_streams;
}

int64_t grdma_h2_deframe(grdma_h2_parser* p, const void* d_arena, const grdma_read_slice* slices,
                         uint64_t n, grdma_h2_event* events_out, uint64_t cap, int* h2_error) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !d_arena || (!slices && n) || !events_out) return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  grdma_h2_deframe_result h_res;
  memset(&h_res, 0, sizeof(h_res));
  static_assert(sizeof(grdma_read_slice) == sizeof(grdma_slice_out), "layout");
  if (!h2_grow(&p->d_sl, &p->sl_cap, n ? n : 1) || !h2_grow(&p->d_ev, &p->ev_cap, cap ? cap : 1))
    return -GRDMA_ERR_HIP;
  hipStream_t st = hc->stream;
  if (n && hipMemcpyAsync(p->d_sl, slices, sizeof(grdma_slice_out) * n, hipMemcpyHostToDevice, st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  const bool chunked = n >= H2_CHUNK_MIN_SLICES && h2_chunks_prepare(p, cap, st);
  hipEventRecord(hc->e0, st);
  const hipError_t launched =
      h2_launch(h2_stage_deframe(p, static_cast<const uint8_t*>(d_arena), p->d_sl, n, p->d_ev, cap, p->d_res, chunked), st);
  hipEventRecord(hc->e1, st);
  if (launched != hipSuccess ||
      hipMemcpyAsync(&h_res, p->d_res, sizeof(h_res), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  float ms = 0;
  if (hipEventElapsedTime(&ms, hc->e0, hc->e1) == hipSuccess) g_h2_last_kernel_us = 1e3 * ms;
  g_h2_last_boundary_steps = h_res.boundary_steps;
  {
    const uint64_t st[8] = {h_res.bulk_steps, h_res.bulk_frames, h_res.boundary_steps, h_res.t_wait,
                            h_res.t_bulk, h_res.t_boundary, h_res.t_serial, h_res.t_total};
    for (int i = 0; i < 8; i++) g_h2_last_stats[i] = st[i];
  }
  const uint64_t m = h_res.nevents < cap ? h_res.nevents : cap;
  if (m && (hipMemcpyAsync(events_out, p->d_ev, sizeof(grdma_h2_event) * m, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess))
    return -GRDMA_ERR_HIP;
  if (h2_error) *h2_error = (int)h_res.error;
  p->standalone_calls++;
  p->standalone_ev_cap = cap;
  return h_res.overflow ? -GRDMA_ERR_CAPACITY : (int64_t)m;
}

// ---- the delivered slices of many transports in one launch (k_h2_deframe_links) ---------------------------------
// One device block per process holds a call: [table | slice lists | zeroed results] go up in one copy, [results | event
// segments] come down in one copy, the kernel in between.  Nothing per item returns to the host.  The download moves
// every item's whole event capacity, not the events produced (their number is only known behind it): callers give
// tight caps.  The block is process-global and unguarded: one call at a time (as the other grdma_h2_* calls, which share
// one stream and its timing events).
namespace {
struct h2_batch_buf {
  uint8_t* d = nullptr;
  uint64_t cap = 0;
};
h2_batch_buf g_batch;
bool h2_batch_reserve(uint64_t total, hipStream_t st) {
  if (total <= g_batch.cap) return true;
  if (hipStreamSynchronize(st) != hipSuccess) return false;  // (the previous call's block goes)
  hipFree(g_batch.d);
  g_batch.d = nullptr;
  g_batch.cap = 0;
  uint64_t want = 1 << 16;
  while (want < total) want *= 2;
  if (hipMalloc((void**)&g_batch.d, want) != hipSuccess) return false;
  g_batch.cap = want;
  return true;
}
}  // namespace

int grdma_h2_deframe_batch(grdma_h2_deframe_item* items, uint32_t n_items) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!items || n_items == 0 || n_items > GRDMA_H2_BATCH_MAX) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 batch: 1 .. GRDMA_H2_BATCH_MAX items");
  uint64_t n_sl = 0, n_ev = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_deframe_item& it = items[i];
    if (!it.parser || !it.d_arena || (!it.slices && it.n) || (!it.events_out && it.cap))
      return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 batch: an item without parser, arena, slices or event array");
    if (it.parser->asm_attached) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 batch: a parser whose assembler is attached to a pipe");
    if (it.parser->fc) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 batch: a parser with a flow-control ledger (single transport only)");
    for (uint32_t k = 0; k < i; k++)
      if (items[k].parser == it.parser) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 batch: the same parser twice");
    n_sl += it.n;
    n_ev += it.cap;
  }
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  hipStream_t st = hc->stream;
  // layout (every part 16-byte aligned): table, slice lists, results, event segments
  auto up16 = [](uint64_t v) { return (v + 15) & ~15ull; };
  const uint64_t o_sl = up16(sizeof(grdma_h2_link_deframe) * n_items);
  const uint64_t o_res = o_sl + sizeof(grdma_slice_out) * n_sl;
  const uint64_t o_ev = up16(o_res + sizeof(grdma_h2_deframe_result) * n_items);
  const uint64_t total = o_ev + sizeof(grdma_h2_event) * n_ev + 16;
  if (!h2_batch_reserve(total, st)) return -GRDMA_ERR_HIP;
  uint8_t* const d = g_batch.d;
  std::vector<uint8_t> up(o_ev, 0), down(total - o_res);  // (the result blocks go up zeroed: a call never reports another's)
  auto* tab = reinterpret_cast<grdma_h2_link_deframe*>(up.data());
  auto* sl = reinterpret_cast<grdma_slice_out*>(up.data() + o_sl);
  static_assert(sizeof(grdma_read_slice) == sizeof(grdma_slice_out), "layout");
  uint64_t a_sl = 0, a_ev = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_deframe_item& it = items[i];
    if (it.n) memcpy(sl + a_sl, it.slices, sizeof(grdma_slice_out) * it.n);
    tab[i].n_step = nullptr;  // (the caller's list: its length is the count)
    tab[i].res = reinterpret_cast<grdma_h2_deframe_result*>(d + o_res) + i;
    tab[i].gp = it.parser->d;
    tab[i].arena = static_cast<const uint8_t*>(it.d_arena);
    tab[i].slices = reinterpret_cast<const grdma_slice_out*>(d + o_sl) + a_sl;
    tab[i].nslices = it.n;
    tab[i].ev = reinterpret_cast<grdma_h2_event*>(d + o_ev) + a_ev;
    tab[i].ev_cap = it.cap;
    a_sl += it.n;
    a_ev += it.cap;
  }
  // behind each parser's previous deframing (a pipe step on another stream)
  for (uint32_t i = 0; i < n_items; i++)
    if (!h2_wait_parser(st, items[i].parser)) return -GRDMA_ERR_HIP;
  if (hipMemcpyAsync(d, up.data(), o_ev, hipMemcpyHostToDevice, st) != hipSuccess) return -GRDMA_ERR_HIP;
  hipEventRecord(hc->e0, st);
  if (h2_launch(h2_stage_deframe_links((const grdma_h2_link_deframe*)d, n_items), st) != hipSuccess) {
    hipStreamSynchronize(st);
    return grdma_fail_msg(GRDMA_ERR_HIP, "h2 batch: the launch of k_h2_deframe_links was rejected");
  }
  hipEventRecord(hc->e1, st);
  if (hipMemcpyAsync(down.data(), d + o_res, total - o_res, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  float ms = 0;
  if (hipEventElapsedTime(&ms, hc->e0, hc->e1) == hipSuccess) g_h2_last_kernel_us = 1e3 * ms;
  const auto* res = reinterpret_cast<const grdma_h2_deframe_result*>(down.data());
  const auto* ev = reinterpret_cast<const grdma_h2_event*>(down.data() + (o_ev - o_res));
  a_ev = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    grdma_h2_deframe_item& it = items[i];
    const uint64_t m = res[i].nevents < it.cap ? res[i].nevents : it.cap;
    if (m) memcpy(it.events_out, ev + a_ev, sizeof(grdma_h2_event) * m);
    it.h2_error = (int)res[i].error;
    it.n_events = res[i].overflow ? -(int64_t)GRDMA_ERR_CAPACITY : (int64_t)m;
    a_ev += it.cap;
  }
  return 0;
}

// ---- the message assembler (csrc/grdma_h2_asm.h) -----------------------------------------------------------
struct grdma_h2_asm {
  grdma_h2_parser* parser = nullptr;
  h2a_dev* d = nullptr;
  h2a_dev h;                       // host copy of the configuration words (pointers, capacities)
  h2a_call* d_call = nullptr;      // standalone calls
  uint32_t attached = 0;           // pipes that assemble through it
  uint32_t replies = 0;            // reply framers that read its descriptors (grdma_h2_reply_create)
  uint32_t reply_pipes = 0;        // ... of which in a pipe: their jobs gather from the arena
  hipEvent_t last_read = nullptr;  // the gather of the last reply step enqueued: the next release waits for it
  float plan_ms = 0, copy_ms = 0;  // of the last standalone call
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
};

static void h2_asm_free_scratch(h2a_dev* h) {
  hipFree(h->tiles);
  hipFree(h->keys);
  hipFree(h->comp);
  hipFree(h->msgs);
  hipFree(h->pieces);
  hipFree(h->dtmp);
  hipFree(h->desc);
  h->tiles = nullptr;
  h->keys = nullptr;
  h->comp = nullptr;
  h->msgs = nullptr;
  h->pieces = nullptr;
  h->dtmp = nullptr;
  h->desc = nullptr;
  h->scratch_ev = h->desc_cap = 0;
}

// per-call buffers for calls of up to ev_cap events (a resize drains the device: setup, not a hot path)
static bool h2_asm_prepare(grdma_h2_asm* a, uint64_t ev_cap) {
  ev_cap = (ev_cap + 63) & ~63ull;  // (the kernels work in wave tiles of 64 events)
  if (ev_cap <= a->h.scratch_ev) return true;
  if (hipDeviceSynchronize() != hipSuccess) return false;
  h2a_dev& h = a->h;
  h2_asm_free_scratch(&h);
  const uint64_t tiles = (ev_cap + 63) / 64;
  const uint64_t dcap = ev_cap + (uint64_t)h.tab_mask + 1;
  const bool ok = hipMalloc((void**)&h.tiles, sizeof(h2a_tile) * tiles) == hipSuccess &&
                  hipMalloc((void**)&h.keys, sizeof(h2a_key) * tiles * 64) == hipSuccess &&
                  hipMalloc((void**)&h.comp, sizeof(uint32_t) * tiles * 64) == hipSuccess &&
                  hipMalloc((void**)&h.msgs, sizeof(h2a_msg) * ev_cap) == hipSuccess &&
                  hipMalloc((void**)&h.pieces, sizeof(h2a_piece) * ev_cap) == hipSuccess &&
                  hipMalloc((void**)&h.dtmp, sizeof(grdma_h2_rx_msg) * ev_cap) == hipSuccess &&
                  hipMalloc((void**)&h.desc, sizeof(grdma_h2_rx_msg) * dcap) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    h2_asm_free_scratch(&h);
  } else {
    h.scratch_ev = ev_cap;
    h.desc_cap = dcap;
  }
  // the configuration words only: the ring and the counters stay where the device has them
  return hipMemcpy(&a->d->scratch_ev, &h.scratch_ev, offsetof(h2a_dev, vh) - offsetof(h2a_dev, scratch_ev),
                   hipMemcpyHostToDevice) == hipSuccess && ok;
}

// The descriptors an assembler reports, from its block h as the caller read it behind the assembly: copied to out on st
// (the caller synchronises st when the count is not 0), or with a blocking copy when st is NULL.  Returns their
// number, -GRDMA_ERR_CAPACITY when the call was skipped or they do not fit.
static int64_t h2_asm_descriptors(const h2a_dev& h, grdma_h2_rx_msg* out, uint64_t cap, hipStream_t st) {
  if (h.skip || h.ndesc > cap || h.ndesc > h.desc_cap) return -GRDMA_ERR_CAPACITY;
  const size_t bytes = sizeof(grdma_h2_rx_msg) * h.ndesc;
  if (h.ndesc && (st ? hipMemcpyAsync(out, h.desc, bytes, hipMemcpyDeviceToHost, st)
                     : hipMemcpy(out, h.desc, bytes, hipMemcpyDeviceToHost)) != hipSuccess)
    return -GRDMA_ERR_HIP;
  return (int64_t)h.ndesc;
}

grdma_h2_asm* grdma_h2_asm_create(grdma_h2_parser* parser, void* d_arena, uint64_t arena_bytes,
                                  uint64_t max_message_bytes, uint32_t max_pending) {
  if (grdma_device_count() <= 0 || !parser || !d_arena || arena_bytes < H2A_GRANULE || max_pending == 0 ||
      max_pending >= 0x7fffffffu)
    return nullptr;
  grdma_h2_asm* a = new grdma_h2_asm();
  a->parser = parser;
  memset(&a->h, 0, sizeof(a->h));
  h2a_dev& h = a->h;
  h.arena = static_cast<uint8_t*>(d_arena);
  h.arena_bytes = arena_bytes;
  h.max_msg = max_message_bytes;
  h.max_pending = max_pending;
  h.tab_mask = parser->slots - 1;
  bool ok = hipMalloc((void**)&a->d, sizeof(h2a_dev)) == hipSuccess &&
            hipMalloc((void**)&h.tab, sizeof(h2a_carry) * parser->slots) == hipSuccess &&
            hipMalloc((void**)&h.recs, sizeof(h2a_rec) * max_pending) == hipSuccess &&
            hipMalloc((void**)&h.fin, sizeof(h2a_key) * H2A_LDS_KEYS) == hipSuccess &&
            hipMalloc((void**)&a->d_call, sizeof(h2a_call)) == hipSuccess &&
            hipMemset(h.tab, 0, sizeof(h2a_carry) * parser->slots) == hipSuccess &&
            hipMemcpy(a->d, &h, sizeof(h), hipMemcpyHostToDevice) == hipSuccess &&
            hipEventCreate(&a->e0) == hipSuccess && hipEventCreate(&a->e1) == hipSuccess &&
            hipEventCreate(&a->e2) == hipSuccess;
  if (!ok) {
    grdma_h2_asm_destroy(a);
    return nullptr;
  }
  return a;
}

void grdma_h2_asm_destroy(grdma_h2_asm* a) {
  if (!a || a->attached || a->replies) return;  // (a pipe's graph still runs its kernels on it, a reply reads it: destroy those first)
  hipDeviceSynchronize();
  h2_asm_free_scratch(&a->h);
  hipFree(a->h.tab);
  hipFree(a->h.recs);
  hipFree(a->h.fin);
  hipFree(a->d);
  hipFree(a->d_call);
  for (hipEvent_t e : {a->e0, a->e1, a->e2})
    if (e) hipEventDestroy(e);
  delete a;
}

int64_t grdma_h2_deframe_messages(grdma_h2_parser* p, grdma_h2_asm* a, const void* d_arena,
                                  const grdma_read_slice* slices, uint64_t n,
                                  grdma_h2_event* events_out, uint64_t ev_cap,
                                  grdma_h2_rx_msg* msgs_out, uint64_t msgs_cap, int* h2_error) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !a || a->parser != p || a->attached || !d_arena || (!slices && n) || ev_cap == 0 || (!msgs_out && msgs_cap))
    return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  if (!h2_grow(&p->d_sl, &p->sl_cap, n ? n : 1) || !h2_grow(&p->d_ev, &p->ev_cap, ev_cap) || !h2_asm_prepare(a, ev_cap))
    return -GRDMA_ERR_HIP;
  hipStream_t st = hc->stream;
  const h2a_call call{p->d_ev, p->d_res, p->d_sl, static_cast<const uint8_t*>(d_arena), ev_cap, 0};
  if (hipMemcpyAsync(a->d_call, &call, sizeof(call), hipMemcpyHostToDevice, st) != hipSuccess ||
      (n && hipMemcpyAsync(p->d_sl, slices, sizeof(grdma_slice_out) * n, hipMemcpyHostToDevice, st) != hipSuccess))
    return -GRDMA_ERR_HIP;
  const bool chunked = n >= H2_CHUNK_MIN_SLICES && h2_chunks_prepare(p, ev_cap, st);
  hipError_t launched = h2_launch(h2_stage_deframe(p, static_cast<const uint8_t*>(d_arena), p->d_sl, n, p->d_ev, ev_cap, p->d_res, chunked), st);
  // the assembly: the plan, then the copy, timed apart
  const h2_stage assembly = h2_stage_asm(a->d, a->d_call);
  hipEventRecord(a->e0, st);
  if (launched == hipSuccess) launched = h2_launch(assembly.data(), H2_ASM_PLAN, st);
  hipEventRecord(a->e1, st);
  if (launched == hipSuccess) launched = h2_launch(assembly.data() + H2_ASM_PLAN, assembly.size() - H2_ASM_PLAN, st);
  hipEventRecord(a->e2, st);
  grdma_h2_deframe_result h_res;
  h2a_dev h;
  if (launched != hipSuccess || hipMemcpyAsync(&h_res, p->d_res, sizeof(h_res), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(&h, a->d, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  if (hipEventElapsedTime(&a->plan_ms, a->e0, a->e1) != hipSuccess) a->plan_ms = 0;
  if (hipEventElapsedTime(&a->copy_ms, a->e1, a->e2) != hipSuccess) a->copy_ms = 0;
  p->standalone_calls++;
  p->standalone_ev_cap = ev_cap;
  if (h2_error) *h2_error = (int)h_res.error;
  const uint64_t m = h_res.nevents < ev_cap ? h_res.nevents : ev_cap;
  if (events_out && m &&
      (hipMemcpyAsync(events_out, p->d_ev, sizeof(grdma_h2_event) * m, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipStreamSynchronize(st) != hipSuccess))
    return -GRDMA_ERR_HIP;
  if (h_res.overflow) return -GRDMA_ERR_CAPACITY;
  const int64_t nmsgs = h2_asm_descriptors(h, msgs_out, msgs_cap, st);
  if (nmsgs > 0 && hipStreamSynchronize(st) != hipSuccess) return -GRDMA_ERR_HIP;
  return nmsgs;
}

int grdma_h2_asm_release(grdma_h2_asm* a, uint64_t count) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!a || a->attached) return -GRDMA_ERR_INVALID;  // (a pipe step releases everything reported before it itself)
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  // behind the last standalone call (same stream) and the last pipe step of the parser
  if (!h2_wait_parser(hc->stream, a->parser)) return -GRDMA_ERR_HIP;
  const grdma_job_hook release = h2_rec(k_h2_asm_release, 1, 64, a->d, count);
  return h2_launch(&release, 1, hc->stream) == hipSuccess ? 0 : -GRDMA_ERR_HIP;
}

int grdma_h2_asm_stats(grdma_h2_asm* a, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!a || !out) return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  h2a_dev h;
  if (!h2_wait_parser(hc->stream, a->parser)) return -GRDMA_ERR_HIP;
  if (hipMemcpyAsync(&h, a->d, sizeof(h), hipMemcpyDeviceToHost, hc->stream) != hipSuccess ||
      hipStreamSynchronize(hc->stream) != hipSuccess)
    return -GRDMA_ERR_HIP;
  out[0] = h.st_reported;
  out[1] = h.st_ok_bytes;
  out[2] = h.st_too_large;
  out[3] = h.st_no_space;
  out[4] = h.st_trunc;
  out[5] = h.vh - h.vt;
  out[6] = (uint64_t)(a->plan_ms * 1e3f);
  out[7] = (uint64_t)(a->copy_ms * 1e3f);
  return 0;
}

// ---- replies framed from the descriptors (csrc/grdma_h2_reply.h) ---------------------------------------------
struct h2_step_seq;
struct grdma_h2_reply {
  grdma_h2_asm* src = nullptr;
  h2r_dev* d = nullptr;
  h2r_dev h;                        // host copy of the configuration words
  grdma_h2_route* d_routes = nullptr;
  h2_step_seq* seq = nullptr;       // the steps of the reply pipe, single or group, that frames through it (at most one: the scratch is one call's)
  hipEvent_t e0 = nullptr, e1 = nullptr;
};

// where the calls frame to, and (a pipe) the shape they must have: the words of h2r_dev from `out` to the result block
static bool h2_reply_set_target(grdma_h2_reply* r, grdma_sge* out, uint64_t cap, uint8_t* hdr, uint64_t hdr_cap,
                                uint64_t check_shape, uint64_t want_slices, uint64_t want_wire, hipStream_t st) {
  h2r_dev& h = r->h;
  h.out = out;
  h.cap = cap;
  h.hdr = hdr;
  h.hdr_cap = hdr_cap;
  h.check_shape = check_shape;
  h.want_slices = want_slices;
  h.want_wire = want_wire;
  const size_t off = offsetof(h2r_dev, out), len = offsetof(h2r_dev, res) - off;
  uint8_t* dst = reinterpret_cast<uint8_t*>(r->d) + off;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(&h) + off;
  return (st ? hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, st) : hipMemcpy(dst, src, len, hipMemcpyHostToDevice)) ==
         hipSuccess;
}

static bool h2_reply_result(grdma_h2_reply* r, grdma_h2_frame_result* fr) {
  uint64_t res[8];
  if (hipMemcpy(res, reinterpret_cast<uint8_t*>(r->d) + offsetof(h2r_dev, res), sizeof(res), hipMemcpyDeviceToHost) != hipSuccess)
    return false;
  fr->nslices = res[H2R_SLICES];
  fr->hdr_bytes = res[H2R_HDR_BYTES];
  fr->wire_bytes = res[H2R_WIRE_BYTES];
  fr->overflow = res[H2R_OVERFLOW];
  return true;
}

grdma_h2_reply* grdma_h2_reply_create(grdma_h2_asm* source, const grdma_h2_route* routes, uint32_t n_routes,
                                      uint32_t max_frame, uint64_t max_messages) {
  if (grdma_device_count() <= 0 || !source || max_frame == 0 || max_frame >= (1u << 24) || max_messages == 0 ||
      max_messages >= (1ull << 32) || n_routes > H2R_MAX_ROUTES || (n_routes && !routes))
    return nullptr;
  std::vector<grdma_h2_route> tab(routes, routes + n_routes);
  std::sort(tab.begin(), tab.end(), [](const grdma_h2_route& a, const grdma_h2_route& b) { return a.from_stream < b.from_stream; });
  for (uint32_t i = 0; i < n_routes; i++)
    if (tab[i].from_stream == 0 || tab[i].to_stream == 0 || (i && tab[i].from_stream == tab[i - 1].from_stream)) return nullptr;
  grdma_h2_reply* r = new grdma_h2_reply();
  r->src = source;
  source->replies++;
  memset(&r->h, 0, sizeof(r->h));
  h2r_dev& h = r->h;
  h.src = source->d;
  h.n_routes = n_routes;
  h.max_frame = max_frame;
  h.max_messages = max_messages;
  bool ok = hipMalloc((void**)&r->d, sizeof(h2r_dev)) == hipSuccess &&
            hipMalloc((void**)&h.msgs, sizeof(grdma_h2_msg_dev) * max_messages) == hipSuccess &&
            hipMalloc((void**)&h.pos, sizeof(grdma_h2_msg_pos) * max_messages) == hipSuccess &&
            (!n_routes || (hipMalloc((void**)&r->d_routes, sizeof(grdma_h2_route) * n_routes) == hipSuccess &&
                           hipMemcpy(r->d_routes, tab.data(), sizeof(grdma_h2_route) * n_routes, hipMemcpyHostToDevice) == hipSuccess));
  h.routes = r->d_routes;
  ok = ok && hipMemcpy(r->d, &h, sizeof(h), hipMemcpyHostToDevice) == hipSuccess && hipEventCreate(&r->e0) == hipSuccess &&
       hipEventCreate(&r->e1) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    grdma_h2_reply_destroy(r);
    return nullptr;
  }
  return r;
}

void grdma_h2_reply_destroy(grdma_h2_reply* r) {
  if (!r || r->seq) return;  // (the pipe's graph still runs the kernels on it: destroy the pipe first)
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);  // (standalone calls)
  r->src->replies--;
  hipFree(r->h.msgs);
  hipFree(r->h.pos);
  hipFree(r->d_routes);
  hipFree(r->d);
  for (hipEvent_t e : {r->e0, r->e1})
    if (e) hipEventDestroy(e);
  delete r;
}

int64_t grdma_h2_reply_frame(grdma_h2_reply* r, grdma_slice* d_slices_out, uint64_t slices_cap, void* d_hdr_arena,
                             uint64_t hdr_cap, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!r || !d_slices_out || !slices_cap || !d_hdr_arena || !hdr_cap || !out || ((uintptr_t)d_slices_out & 15) ||
      ((uintptr_t)d_hdr_arena & 15) || r->seq || r->src->attached)
    return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  // the stream of grdma_h2_deframe_messages: the call is ordered behind the one it reads
  hipStream_t st = hc->stream;
  if (!h2_reply_set_target(r, reinterpret_cast<grdma_sge*>(d_slices_out), slices_cap, static_cast<uint8_t*>(d_hdr_arena),
                           hdr_cap, 0, 0, 0, st))
    return -GRDMA_ERR_HIP;
  hipEventRecord(r->e0, st);
  const hipError_t launched = h2_launch(h2_stage_reply(r->d), st);
  hipEventRecord(r->e1, st);
  uint64_t res[8];
  if (launched != hipSuccess ||
      hipMemcpyAsync(res, reinterpret_cast<uint8_t*>(r->d) + offsetof(h2r_dev, res), sizeof(res), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  float ms = 0;
  for (int i = 0; i < 7; i++) out[i] = res[i];
  out[7] = hipEventElapsedTime(&ms, r->e0, r->e1) == hipSuccess ? (uint64_t)(ms * 1e3f) : 0;
  if (res[H2R_OVERFLOW]) return -GRDMA_ERR_CAPACITY;
  return (int64_t)res[H2R_SLICES];
}

// ---- the replies of many transports in two launches (h2_stage_reply_links) ------------------------------------------
// The batch block of the process holds the call: [table | one h2r_dev per item] goes up in one copy -- the item's
// framer with the item's targets and a zeroed result block; scratch, routes and source stay the reply's own -- and the
// h2r_dev blocks come down in one copy.  One call at a time, as the other batch calls.

int grdma_h2_reply_frame_batch(grdma_h2_reply_item* items, uint32_t n_items) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!items || n_items == 0 || n_items > GRDMA_H2_BATCH_MAX)
    return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 reply batch: 1 .. GRDMA_H2_BATCH_MAX items");
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_reply_item& it = items[i];
    if (!it.reply) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 reply batch: an item without reply");
    if (!it.d_slices_out || !it.slices_cap || !it.d_hdr_arena || !it.hdr_cap || ((uintptr_t)it.d_slices_out & 15) ||
        ((uintptr_t)it.d_hdr_arena & 15))
      return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 reply batch: a null, zero or misaligned slice table or header arena");
    if (it.reply->seq) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 reply batch: a reply bound to a reply pipe");
    if (it.reply->src->attached)
      return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 reply batch: a source assembler attached to a pipe or group pipe");
    for (uint32_t k = 0; k < i; k++) {
      if (items[k].reply == it.reply) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 reply batch: the same reply twice");
      // (each reply has scratch of its own, so two of one source could run side by side; the rule is one item per
      // transport, as in the other batch calls)
      if (items[k].reply->src == it.reply->src)
        return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 reply batch: two replies of one source assembler");
    }
  }
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  hipStream_t st = hc->stream;
  auto up16 = [](uint64_t v) { return (v + 15) & ~15ull; };
  const uint64_t o_dev = up16(sizeof(h2r_link) * n_items);
  const uint64_t total = o_dev + sizeof(h2r_dev) * n_items;
  if (!h2_batch_reserve(total, st)) return -GRDMA_ERR_HIP;
  uint8_t* const d = g_batch.d;
  std::vector<uint8_t> up(total, 0);
  std::vector<h2r_dev> down(n_items);
  auto* tab = reinterpret_cast<h2r_link*>(up.data());
  auto* devs = reinterpret_cast<h2r_dev*>(up.data() + o_dev);
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_reply_item& it = items[i];
    h2r_dev h = it.reply->h;
    h.out = reinterpret_cast<grdma_sge*>(it.d_slices_out);
    h.cap = it.slices_cap;
    h.hdr = static_cast<uint8_t*>(it.d_hdr_arena);
    h.hdr_cap = it.hdr_cap;
    h.check_shape = h.want_slices = h.want_wire = 0;
    memset(h.res, 0, sizeof(h.res));
    devs[i] = h;
    tab[i].R = reinterpret_cast<h2r_dev*>(d + o_dev) + i;
  }
  // behind each source parser's last deframing (a pipe step on another stream; the standalone calls share this stream)
  for (uint32_t i = 0; i < n_items; i++)
    if (!h2_wait_parser(st, items[i].reply->src->parser)) return -GRDMA_ERR_HIP;
  if (hipMemcpyAsync(d, up.data(), total, hipMemcpyHostToDevice, st) != hipSuccess) return -GRDMA_ERR_HIP;
  hipEventRecord(hc->e0, st);
  if (h2_launch(h2_stage_reply_links((const h2r_link*)d, n_items), st) != hipSuccess) {
    hipStreamSynchronize(st);
    return grdma_fail_msg(GRDMA_ERR_HIP, "h2 reply batch: a launch was rejected");
  }
  hipEventRecord(hc->e1, st);
  if (hipMemcpyAsync(down.data(), d + o_dev, sizeof(h2r_dev) * n_items, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  float ms = 0;
  const uint64_t us = hipEventElapsedTime(&ms, hc->e0, hc->e1) == hipSuccess ? (uint64_t)(ms * 1e3f) : 0;
  g_h2_last_kernel_us = 1e3 * ms;
  for (uint32_t i = 0; i < n_items; i++) {
    grdma_h2_reply_item& it = items[i];
    const uint64_t* res = down[i].res;
    for (int k = 0; k < 7; k++) it.out[k] = res[k];
    it.out[7] = us;  // (the batch's, repeated)
    it.n_slices = res[H2R_OVERFLOW] ? -(int64_t)GRDMA_ERR_CAPACITY : (int64_t)res[H2R_SLICES];
  }
  return 0;
}

// ---- receive flow control: the window ledger (csrc/grdma_h2_fc.h) -------------------------------------------------
struct grdma_h2_pipe;
struct grdma_h2_fc {
  grdma_h2_parser* parser = nullptr;
  h2fc_dev* d = nullptr;
  h2fc_dev h;                      // host copy of the configuration words
  h2fc_call* d_call = nullptr;     // standalone calls
  grdma_h2_pipe* pipe = nullptr;   // the pipe whose steps account through it
  uint64_t accounted = 0;          // parser->standalone_calls of the last call accounted
  float last_ms = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};

// The parser of f is being destroyed: standalone calls on f's stream have ended, and from now on f refuses every call
// but destroy (its device block points into the parser's).  A ledger attached to a pipe stays with the pipe, whose
// parser must outlive it as it must without a ledger.
static void h2_fc_parser_gone(grdma_h2_fc* f) {
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);
  f->parser = nullptr;
}

// the bit words of calls of up to ev_cap events (a resize drains the device: setup, not a hot path)
static bool h2_fc_prepare(grdma_h2_fc* f, uint64_t ev_cap) {
  if (ev_cap == 0) ev_cap = 1;
  if (ev_cap <= f->h.scratch_ev) return true;
  if (ev_cap >= 0xffffffffull) return false;  // (event indices are 32 bits in the scratch table)
  if (hipDeviceSynchronize() != hipSuccess) return false;
  h2fc_dev& h = f->h;
  hipFree(h.mark);
  hipFree(h.mark_pre);
  h.mark = h.mark_pre = nullptr;
  h.scratch_ev = 0;
  const uint64_t words = (ev_cap + 31) / 32;
  const bool ok = hipMalloc((void**)&h.mark, sizeof(uint32_t) * words) == hipSuccess &&
                  hipMalloc((void**)&h.mark_pre, sizeof(uint32_t) * words) == hipSuccess;
  if (ok) h.scratch_ev = ev_cap;
  else (void)hipGetLastError();
  const size_t off = offsetof(h2fc_dev, scratch_ev), len = offsetof(h2fc_dev, out) - off;
  return hipMemcpy(reinterpret_cast<uint8_t*>(f->d) + off, reinterpret_cast<const uint8_t*>(&h) + off, len,
                   hipMemcpyHostToDevice) == hipSuccess && ok;
}

// where the calls write: the words of h2fc_dev from `out` to the state
static bool h2_fc_set_target(grdma_h2_fc* f, grdma_sge* out, uint64_t cap, uint8_t* hdr, uint64_t hdr_cap, hipStream_t st) {
  h2fc_dev& h = f->h;
  h.out = out;
  h.cap = cap;
  h.hdr = hdr;
  h.hdr_cap = hdr_cap;
  const size_t off = offsetof(h2fc_dev, out), len = offsetof(h2fc_dev, announced) - off;
  uint8_t* dst = reinterpret_cast<uint8_t*>(f->d) + off;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(&h) + off;
  return (st ? hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, st) : hipMemcpy(dst, src, len, hipMemcpyHostToDevice)) ==
         hipSuccess;
}

static grdma_h2_fc* h2_fc_refuse(const char* why) {
  grdma_fail_msg(GRDMA_ERR_INVALID, why);
  return nullptr;
}

grdma_h2_fc* grdma_h2_fc_create(grdma_h2_parser* parser, uint32_t stream_window, uint32_t conn_window, uint32_t conn_threshold,
                                uint32_t max_updates) {
  if (grdma_device_count() <= 0) return nullptr;
  if (!parser) return h2_fc_refuse("h2 flow control: no parser");
  if (parser->fc) return h2_fc_refuse("h2 flow control: the parser has a ledger already");
  if (stream_window == 0 || stream_window > 0x7fffffffu) return h2_fc_refuse("h2 flow control: stream_window outside 1 .. 2^31 - 1");
  if (conn_window < 65535 || conn_window > 0x7fffffffu) return h2_fc_refuse("h2 flow control: conn_window outside 65535 .. 2^31 - 1");
  if (conn_threshold > conn_window) return h2_fc_refuse("h2 flow control: conn_threshold above conn_window");
  if (max_updates == 0 || max_updates > (1u << 24)) return h2_fc_refuse("h2 flow control: max_updates outside 1 .. 2^24");
  grdma_h2_fc* f = new grdma_h2_fc();
  f->parser = parser;
  memset(&f->h, 0, sizeof(f->h));
  h2fc_dev& h = f->h;
  h.gp = parser->d;
  h.stream_window = stream_window;
  h.conn_window = conn_window;
  h.conn_threshold = conn_threshold;
  h.max_updates = max_updates;
  h.tab_mask = parser->slots - 1;
  h.announced = (int64_t)conn_window;
  const bool ok = hipMalloc((void**)&f->d, sizeof(h2fc_dev)) == hipSuccess &&
                  hipMalloc((void**)&h.tab, sizeof(h2fc_slot) * parser->slots) == hipSuccess &&
                  hipMalloc((void**)&h.upd, sizeof(h2fc_upd) * max_updates) == hipSuccess &&
                  hipMalloc((void**)&f->d_call, sizeof(h2fc_call)) == hipSuccess &&
                  hipMemcpy(f->d, &h, sizeof(h), hipMemcpyHostToDevice) == hipSuccess &&
                  hipEventCreate(&f->e0) == hipSuccess && hipEventCreate(&f->e1) == hipSuccess;
  parser->fc = f;
  if (!ok) {
    (void)hipGetLastError();
    grdma_h2_fc_destroy(f);
    grdma_fail_msg(GRDMA_ERR_HIP, "h2 flow control: device allocation failed");
    return nullptr;
  }
  return f;
}

void grdma_h2_fc_destroy(grdma_h2_fc* f) {
  if (!f || f->pipe) return;  // (the pipe's graph still runs the kernels on it: destroy the pipe first)
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);  // (standalone calls)
  if (f->parser) f->parser->fc = nullptr;
  hipFree(f->h.tab);
  hipFree(f->h.upd);
  hipFree(f->h.mark);
  hipFree(f->h.mark_pre);
  hipFree(f->d);
  hipFree(f->d_call);
  for (hipEvent_t e : {f->e0, f->e1})
    if (e) hipEventDestroy(e);
  delete f;
}

int64_t grdma_h2_fc_account(grdma_h2_fc* f, grdma_slice* d_slices_out, uint64_t slices_cap, void* d_hdr_arena, uint64_t hdr_cap,
                            uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!f || !out) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 flow control: no ledger or no result array");
  if (!d_slices_out || !slices_cap || !d_hdr_arena || !hdr_cap || ((uintptr_t)d_slices_out & 15) || ((uintptr_t)d_hdr_arena & 15))
    return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 flow control: a null, zero or misaligned slice table or header arena");
  if (f->pipe) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 flow control: the ledger is attached to a pipe (its steps account)");
  grdma_h2_parser* p = f->parser;
  if (!p) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 flow control: the ledger's parser is gone");
  if (p->standalone_calls == 0) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 flow control: the parser has deframed nothing yet");
  if (f->accounted == p->standalone_calls) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 flow control: this call is accounted already");
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  if (!h2_fc_prepare(f, p->standalone_ev_cap)) return -GRDMA_ERR_HIP;
  // the stream of the standalone deframings: the call is ordered behind the one it reads
  // ... and behind the parser's last deframing by a pipe: k_h2_fc_finish reads the stream map that step may change
  hipStream_t st = hc->stream;
  if (!h2_wait_parser(st, p)) return -GRDMA_ERR_HIP;
  const h2fc_call call{p->d_ev, p->d_res, p->standalone_ev_cap};
  if (hipMemcpyAsync(f->d_call, &call, sizeof(call), hipMemcpyHostToDevice, st) != hipSuccess ||
      !h2_fc_set_target(f, reinterpret_cast<grdma_sge*>(d_slices_out), slices_cap, static_cast<uint8_t*>(d_hdr_arena), hdr_cap, st))
    return -GRDMA_ERR_HIP;
  hipEventRecord(f->e0, st);
  const hipError_t launched = h2_launch(h2_stage_fc(f->d, f->d_call), st);
  hipEventRecord(f->e1, st);
  uint64_t res[8];
  if (launched != hipSuccess ||
      hipMemcpyAsync(res, reinterpret_cast<uint8_t*>(f->d) + offsetof(h2fc_dev, res), sizeof(res), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  if (hipEventElapsedTime(&f->last_ms, f->e0, f->e1) != hipSuccess) f->last_ms = 0;
  f->accounted = p->standalone_calls;
  for (int i = 0; i < 8; i++) out[i] = res[i];
  if (res[H2FC_OVERFLOW] == 2)
    return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 flow control: the call's event list overflowed, its bytes cannot be accounted");
  if (res[H2FC_OVERFLOW]) return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 flow control: more frames than max_updates, or a slice or header cap too small");
  return (int64_t)res[H2FC_SLICES];
}

int grdma_h2_fc_stats(grdma_h2_fc* f, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!f || !out) return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  h2fc_dev h;
  if (f->parser && !h2_wait_parser(hc->stream, f->parser)) return -GRDMA_ERR_HIP;
  if (hipMemcpyAsync(&h, f->d, sizeof(h), hipMemcpyDeviceToHost, hc->stream) != hipSuccess ||
      hipStreamSynchronize(hc->stream) != hipSuccess)
    return -GRDMA_ERR_HIP;
  out[0] = h.st_calls;
  out[1] = h.st_conn_bytes;
  out[2] = h.st_stream_bytes;
  out[3] = h.st_frames;
  out[4] = h.st_conn_over;
  out[5] = h.st_stream_over | (h.lost ? 1ull << 63 : 0);
  out[6] = (uint64_t)h.announced;
  out[7] = (uint64_t)(f->last_ms * 1e6f);
  return 0;
}

// ---- the message assembler on many links (h2_stage_asm_links, csrc/grdma_h2_asm.h) ---------------------------------

namespace {
// timing events of the batched assembly (plan | copy) and the pinned table of grdma_h2_asm_release_batch with the event
// of its last upload (the table is reused: the next call waits for that upload)
struct h2_links_ctx {
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, rel_up = nullptr;
  h2a_link_release* h_rel = nullptr;
  h2a_link_release* d_rel = nullptr;
  bool rel_pending = false;
};
h2_links_ctx* h2_links() {
  static h2_links_ctx c;
  static const bool ok = hipEventCreate(&c.e0) == hipSuccess && hipEventCreate(&c.e1) == hipSuccess &&
                         hipEventCreate(&c.e2) == hipSuccess &&
                         hipEventCreateWithFlags(&c.rel_up, hipEventDisableTiming) == hipSuccess &&
                         hipHostMalloc((void**)&c.h_rel, sizeof(h2a_link_release) * GRDMA_H2_BATCH_MAX) == hipSuccess &&
                         hipMalloc((void**)&c.d_rel, sizeof(h2a_link_release) * GRDMA_H2_BATCH_MAX) == hipSuccess;
  return ok ? &c : nullptr;
}
}  // namespace

int grdma_h2_deframe_messages_batch(grdma_h2_messages_item* items, uint32_t n_items) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!items || n_items == 0 || n_items > GRDMA_H2_BATCH_MAX)
    return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 messages batch: 1 .. GRDMA_H2_BATCH_MAX items");
  uint64_t n_sl = 0, n_ev = 0;
  bool want_events = false;
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_messages_item& it = items[i];
    if (!it.parser || !it.d_arena || (!it.slices && it.n) || it.cap == 0 || (!it.msgs_out && it.msgs_cap))
      return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 messages batch: an item without parser, arena, slices, event capacity or descriptor array");
    if (!it.assembler) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 messages batch: an item without assembler");
    if (it.assembler->parser != it.parser) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 messages batch: an assembler of another parser");
    if (it.parser->fc) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 messages batch: a parser with a flow-control ledger (single transport only)");
    if (it.assembler->attached || it.parser->asm_attached)
      return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 messages batch: an assembler attached to a pipe");
    for (uint32_t k = 0; k < i; k++) {
      if (items[k].parser == it.parser) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 messages batch: the same parser twice");
      if (items[k].assembler == it.assembler) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 messages batch: the same assembler twice");
    }
    n_sl += it.n;
    n_ev += it.cap;
    want_events = want_events || it.events_out;
  }
  h2_host_ctx* hc = h2_ctx();
  h2_links_ctx* lc = h2_links();
  if (!hc || !lc) return -GRDMA_ERR_HIP;
  hipStream_t st = hc->stream;
  for (uint32_t i = 0; i < n_items; i++)
    if (!h2_asm_prepare(items[i].assembler, items[i].cap)) return -GRDMA_ERR_HIP;
  // layout (every part 16-byte aligned): deframe table, assembler table, call blocks, slice lists, results, event segments
  auto up16 = [](uint64_t v) { return (v + 15) & ~15ull; };
  const uint64_t o_atab = up16(sizeof(grdma_h2_link_deframe) * n_items);
  const uint64_t o_call = o_atab + up16(sizeof(h2a_link) * n_items);
  const uint64_t o_sl = o_call + up16(sizeof(h2a_call) * n_items);
  const uint64_t o_res = o_sl + sizeof(grdma_slice_out) * n_sl;
  const uint64_t o_ev = up16(o_res + sizeof(grdma_h2_deframe_result) * n_items);
  const uint64_t total = o_ev + sizeof(grdma_h2_event) * n_ev + 16;
  if (!h2_batch_reserve(total, st)) return -GRDMA_ERR_HIP;
  uint8_t* const d = g_batch.d;
  // (the result blocks go up zeroed; the events come down only when an item asks for them)
  std::vector<uint8_t> up(o_ev, 0), down((want_events ? total : o_ev) - o_res);
  auto* dtab = reinterpret_cast<grdma_h2_link_deframe*>(up.data());
  auto* atab = reinterpret_cast<h2a_link*>(up.data() + o_atab);
  auto* calls = reinterpret_cast<h2a_call*>(up.data() + o_call);
  auto* sl = reinterpret_cast<grdma_slice_out*>(up.data() + o_sl);
  static_assert(sizeof(grdma_read_slice) == sizeof(grdma_slice_out), "layout");
  uint64_t a_sl = 0, a_ev = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_messages_item& it = items[i];
    if (it.n) memcpy(sl + a_sl, it.slices, sizeof(grdma_slice_out) * it.n);
    grdma_h2_link_deframe& q = dtab[i];
    q.n_step = nullptr;  // (the caller's list: its length is the count)
    q.res = reinterpret_cast<grdma_h2_deframe_result*>(d + o_res) + i;
    q.gp = it.parser->d;
    q.arena = static_cast<const uint8_t*>(it.d_arena);
    q.slices = reinterpret_cast<const grdma_slice_out*>(d + o_sl) + a_sl;
    q.nslices = it.n;
    q.ev = reinterpret_cast<grdma_h2_event*>(d + o_ev) + a_ev;
    q.ev_cap = it.cap;
    calls[i] = h2a_call{q.ev, q.res, q.slices, q.arena, it.cap, 0};
    atab[i].A = it.assembler->d;
    atab[i].call = reinterpret_cast<const h2a_call*>(d + o_call) + i;
    a_sl += it.n;
    a_ev += it.cap;
  }
  // behind each parser's previous deframing (a pipe step on another stream)
  for (uint32_t i = 0; i < n_items; i++)
    if (!h2_wait_parser(st, items[i].parser)) return -GRDMA_ERR_HIP;
  if (hipMemcpyAsync(d, up.data(), o_ev, hipMemcpyHostToDevice, st) != hipSuccess) return -GRDMA_ERR_HIP;
  hipEventRecord(hc->e0, st);
  hipError_t launched = h2_launch(h2_stage_deframe_links((const grdma_h2_link_deframe*)d, n_items), st);
  hipEventRecord(hc->e1, st);
  // the assembly: the plan, then the copy, timed apart
  const h2_stage assembly = h2_stage_asm_links(reinterpret_cast<const h2a_link*>(d + o_atab), n_items);
  hipEventRecord(lc->e0, st);
  if (launched == hipSuccess) launched = h2_launch(assembly.data(), H2_ASM_PLAN, st);
  hipEventRecord(lc->e1, st);
  if (launched == hipSuccess) launched = h2_launch(assembly.data() + H2_ASM_PLAN, assembly.size() - H2_ASM_PLAN, st);
  hipEventRecord(lc->e2, st);
  if (launched != hipSuccess) {
    hipStreamSynchronize(st);
    return grdma_fail_msg(GRDMA_ERR_HIP, "h2 messages batch: a launch was rejected");
  }
  // one download of the results (and the events); then every assembler's block, and the descriptors from where each
  // assembler keeps them (its own buffer: the kernels are the single call's, which reports from there)
  std::vector<h2a_dev> hs(n_items);
  if (hipMemcpyAsync(down.data(), d + o_res, down.size(), hipMemcpyDeviceToHost, st) != hipSuccess) return -GRDMA_ERR_HIP;
  for (uint32_t i = 0; i < n_items; i++)
    if (hipMemcpyAsync(&hs[i], items[i].assembler->d, sizeof(h2a_dev), hipMemcpyDeviceToHost, st) != hipSuccess) return -GRDMA_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess) return -GRDMA_ERR_HIP;
  float ms = 0, plan_ms = 0, copy_ms = 0;
  if (hipEventElapsedTime(&ms, hc->e0, hc->e1) == hipSuccess) g_h2_last_kernel_us = 1e3 * ms;
  if (hipEventElapsedTime(&plan_ms, lc->e0, lc->e1) != hipSuccess) plan_ms = 0;
  if (hipEventElapsedTime(&copy_ms, lc->e1, lc->e2) != hipSuccess) copy_ms = 0;
  const auto* res = reinterpret_cast<const grdma_h2_deframe_result*>(down.data());
  const auto* ev = reinterpret_cast<const grdma_h2_event*>(down.data() + (o_ev - o_res));
  a_ev = 0;
  bool more = false;
  for (uint32_t i = 0; i < n_items; i++) {
    grdma_h2_messages_item& it = items[i];
    const uint64_t m = res[i].nevents < it.cap ? res[i].nevents : it.cap;
    if (it.events_out && m) memcpy(it.events_out, ev + a_ev, sizeof(grdma_h2_event) * m);
    it.h2_error = (int)res[i].error;
    it.n_events = res[i].overflow ? -(int64_t)GRDMA_ERR_CAPACITY : (int64_t)m;
    it.assembler->plan_ms = plan_ms;  // (the batch's, repeated)
    it.assembler->copy_ms = copy_ms;
    it.n_msgs = res[i].overflow ? -(int64_t)GRDMA_ERR_CAPACITY : h2_asm_descriptors(hs[i], it.msgs_out, it.msgs_cap, st);
    if (it.n_msgs == -(int64_t)GRDMA_ERR_HIP) return -GRDMA_ERR_HIP;
    more = more || it.n_msgs > 0;
    a_ev += it.cap;
  }
  if (more && hipStreamSynchronize(st) != hipSuccess) return -GRDMA_ERR_HIP;
  return 0;
}

int grdma_h2_asm_release_batch(grdma_h2_asm* const* asms, const uint64_t* counts, uint32_t n) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!asms || !counts || n == 0 || n > GRDMA_H2_BATCH_MAX)
    return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 release batch: 1 .. GRDMA_H2_BATCH_MAX assemblers");
  for (uint32_t i = 0; i < n; i++) {
    if (!asms[i]) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 release batch: a null assembler");
    if (asms[i]->attached) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 release batch: an assembler attached to a pipe");
    for (uint32_t k = 0; k < i; k++)
      if (asms[k] == asms[i]) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 release batch: the same assembler twice");
  }
  h2_host_ctx* hc = h2_ctx();
  h2_links_ctx* lc = h2_links();
  if (!hc || !lc) return -GRDMA_ERR_HIP;
  hipStream_t st = hc->stream;
  // behind the last standalone call (same stream) and the last pipe step of every parser
  for (uint32_t i = 0; i < n; i++)
    if (!h2_wait_parser(st, asms[i]->parser)) return -GRDMA_ERR_HIP;
  if (lc->rel_pending && hipEventSynchronize(lc->rel_up) != hipSuccess) return -GRDMA_ERR_HIP;
  for (uint32_t i = 0; i < n; i++) lc->h_rel[i] = h2a_link_release{asms[i]->d, counts[i]};
  if (hipMemcpyAsync(lc->d_rel, lc->h_rel, sizeof(h2a_link_release) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipEventRecord(lc->rel_up, st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  lc->rel_pending = true;
  const grdma_job_hook release = h2_rec(k_h2_asm_release_links, n, 64, lc->d_rel);
  return h2_launch(&release, 1, st) == hipSuccess ? 0 : -GRDMA_ERR_HIP;
}

#include "grdma_h2_host_pipe.inc"

}  // extern "C"
