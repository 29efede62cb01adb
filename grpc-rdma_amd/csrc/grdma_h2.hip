// HTTP/2 DATA framing (K6/K7) and deframing (K8/K9) on the device.
//
// TX  k_h2_frame_index + k_h2_frame_emit   build, in HBM, the slice list chttp2 hands to
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

// The deframing of one list of delivered slices, enqueued on st: over chunks when the parser has the buffers (plan,
// the chunks side by side, then the merge -- or the sequential deframer over the whole list when the chain did not hold), else the sequential deframer alone.
static void h2_enqueue_deframe(grdma_h2_parser* p, const uint8_t* arena, const grdma_slice_out* d_slices, uint64_t n,
                               grdma_h2_event* d_ev, uint64_t ev_cap, grdma_h2_deframe_result* d_res, hipStream_t st,
                               bool chunked) {
  if (!chunked || n < H2_CHUNK_MIN_SLICES) {
    hipLaunchKernelGGL(k_h2_deframe, dim3(1), dim3(H2_DEFRAME_THREADS), 0, st, p->d, arena, d_slices, n, d_ev, ev_cap, d_res);
    return;
  }
  hipLaunchKernelGGL(k_h2_deframe_chunks, dim3((unsigned)p->chunks_want), dim3(H2_DEFRAME_THREADS), 0, st, p->d, p->d_chunks,
                     arena, d_slices, n);
  hipLaunchKernelGGL(k_h2_merge_or_deframe, dim3(H2_MERGE_GRID), dim3(H2_DEFRAME_THREADS), 0, st, p->d, p->d_chunks, arena,
                     d_slices, n, d_ev, ev_cap, d_res);
}

// The framing of one message table, enqueued on st: sizes and positions, then one wave per message (grdma_h2_kernels.h).
static void h2_enqueue_frame(const grdma_h2_msg_dev* d_msgs, uint64_t n, uint32_t max_frame, grdma_sge* out, uint64_t cap,
                             uint8_t* hdr, uint64_t hdr_cap, grdma_h2_msg_pos* d_pos, grdma_h2_frame_result* d_res,
                             hipStream_t st) {
  const uint64_t per = H2_EMIT_THREADS / 64;
  if (n <= H2_FRAME_ONE_MAX) {  // one launch: every workgroup sums what lies in front of its messages itself
    hipLaunchKernelGGL(k_h2_frame_one, dim3((unsigned)((n + per - 1) / per)), dim3(H2_EMIT_THREADS), 0, st, d_msgs, n, max_frame,
                       out, cap, hdr, hdr_cap, d_res);
    return;
  }
  hipLaunchKernelGGL(k_h2_frame_index, dim3(1), dim3(256), 0, st, d_msgs, n, max_frame, cap, hdr_cap, d_pos, d_res);
  hipLaunchKernelGGL(k_h2_frame_emit, dim3((unsigned)((n + per - 1) / per)), dim3(H2_EMIT_THREADS), 0, st, d_msgs, n, max_frame,
                     out, cap, hdr, hdr_cap, (const grdma_h2_msg_pos*)d_pos);
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
  std::vector<grdma_h2_msg_dev> tmp(n);
  for (uint64_t i = 0; i < n; i++) {
    tmp[i].payload = static_cast<const uint8_t*>(msgs[i].payload);
    tmp[i].len = msgs[i].len;
    tmp[i].stream_id = msgs[i].stream_id;
    tmp[i].flags = msgs[i].flags;
    if (msgs[i].len >= (1ull << 32)) return -GRDMA_ERR_INVALID;  // 32-bit message length field
  }
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
  h2_enqueue_frame(d_msgs, n, max_frame, reinterpret_cast<grdma_sge*>(d_slices_out), slices_cap,
                   static_cast<uint8_t*>(d_hdr_arena), hdr_cap, d_pos, d_res, st);
  hipEventRecord(hc->e1, st);
  if (hipMemcpyAsync(&h_res, d_res, sizeof(h_res), hipMemcpyDeviceToHost, st) != hipSuccess ||
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

void grdma_h2_parser_destroy(grdma_h2_parser* p) {
  if (!p) return;
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
  h2_enqueue_deframe(p, static_cast<const uint8_t*>(d_arena), p->d_sl, n, p->d_ev, cap, p->d_res, st, chunked);
  hipEventRecord(hc->e1, st);
  if (hipMemcpyAsync(&h_res, p->d_res, sizeof(h_res), hipMemcpyDeviceToHost, st) != hipSuccess ||
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
  for (uint32_t i = 0; i < n_items; i++) {
    grdma_h2_parser* p = items[i].parser;
    if (p->last_deframed && p->last_stream != st && hipStreamWaitEvent(st, p->last_deframed, 0) != hipSuccess) return -GRDMA_ERR_HIP;
  }
  if (hipMemcpyAsync(d, up.data(), o_ev, hipMemcpyHostToDevice, st) != hipSuccess) return -GRDMA_ERR_HIP;
  hipEventRecord(hc->e0, st);
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_h2_deframe_links, dim3(n_items), dim3(H2_DEFRAME_THREADS), 0, st, (const grdma_h2_link_deframe*)d);
  if (hipGetLastError() != hipSuccess) {
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

// ---- HTTP/2 inside the device pipeline ------------------------------------------------------
// frame (k_h2_frame_index + k_h2_frame_emit rebuild the job's slice list from the message table) -> the streaming job
// -> deframe (the deframer over the slices the job delivered), all enqueued.  By default the two stages are kernel
// nodes of the job's own graph (one launch per step); with GRDMA_H2_PIPE_FUSED=0, and under the engine schedule, they
// are enqueued around the job's launch, ordered by events, with per-stage event timing.
struct grdma_stream_job;
int grdma_job_link_view(grdma_stream_job* j, uint32_t link, grdma_sge** d_sges, uint64_t* count,
                        grdma_slice_out** d_slices, uint8_t** dst, hipStream_t* stream);
extern "C" uint32_t grdma_job_link_count(grdma_stream_job* j);
extern "C" int grdma_job_link_step_slices(grdma_stream_job* j, uint32_t link, const uint64_t** d_count, uint64_t* cap);
int grdma_stream_job_launch(grdma_stream_job* j);
extern "C" int grdma_job_set_hooks(grdma_stream_job* j, const grdma_job_hook* pre, uint32_t n_pre, const grdma_job_hook* post,
                                   uint32_t n_post);
extern "C" int grdma_job_hook_counts(grdma_stream_job* j, uint32_t out[2]);

struct grdma_h2_pipe {
  grdma_stream_job* job = nullptr;
  grdma_h2_parser* parser = nullptr;
  grdma_sge* d_sges = nullptr;
  uint64_t count = 0;
  grdma_slice_out* d_slices = nullptr;
  uint8_t* dst = nullptr;
  hipStream_t job_stream = nullptr, frame_stream = nullptr, deframe_stream = nullptr;
  hipEvent_t framed = nullptr, job_done = nullptr, deframed = nullptr;
  hipEvent_t t_f0 = nullptr, t_d0 = nullptr, t_f1 = nullptr, t_d1 = nullptr;  // kernel start / end stamps of the last step
  grdma_h2_msg_dev* d_msgs = nullptr;
  grdma_h2_msg_pos* d_pos = nullptr;
  uint64_t nmsgs = 0;
  uint32_t max_frame = 16384;
  uint8_t* d_hdr = nullptr;
  uint64_t hdr_cap = 0;
  grdma_h2_frame_result* d_fres = nullptr;
  grdma_h2_deframe_result* d_dres = nullptr;
  grdma_h2_event* d_ev = nullptr;
  uint64_t ev_cap = 0, delivered = 0;
  uint64_t boundary_steps = 0, t_boundary = 0;  // of the last synced step
  bool launched = false;
  bool chunked = false;  // the parser has chunk buffers for this pipe's event capacity
  bool fused = false;    // framing and deframing are nodes of the job's graph (one launch per step)
  bool timed = false;    // the last step recorded the per-stage timing events
  grdma_h2_asm* asm_ = nullptr;  // the message assembler behind the deframer (grdma_h2_pipe_attach_assembler)
  h2a_call* d_call = nullptr;    // where this pipe's deframer leaves its output, for the assembler
  grdma_h2_reply* reply = nullptr;  // a reply pipe (grdma_h2_pipe_create_reply): the framing stage is csrc/grdma_h2_reply.h
  grdma_job_hook pre[2], post[2];
  uint32_t n_pre = 0, n_post = 0;
};

namespace {
hipStream_t g_pipe_frame_stream = nullptr, g_pipe_deframe_stream = nullptr;
}
static void h2_asm_detach(grdma_h2_pipe* p);
static void h2_asm_enqueue(grdma_h2_asm* a, const h2a_call* d_call, hipStream_t st);
// reply pipes and the pipes they read from (defined with grdma_h2_reply below)
static bool h2_asm_read_by_reply_pipes(const grdma_h2_asm* a);
static hipEvent_t h2_asm_last_read(const grdma_h2_asm* a);
static bool h2_reply_bind_pipe(grdma_h2_reply* r, grdma_h2_pipe* p, uint64_t recorded_wire_bytes);
static void h2_reply_unbind_pipe(grdma_h2_pipe* p);
static int h2_reply_wait_source(grdma_h2_pipe* p, hipStream_t st);
static void h2_reply_enqueue(grdma_h2_reply* r, hipStream_t st);
static void h2_reply_step_enqueued(grdma_h2_pipe* p, hipEvent_t read_done);
static uint32_t h2_reply_hooks(grdma_h2_reply* r, grdma_job_hook* out);
static bool h2_reply_result(grdma_h2_reply* r, grdma_h2_frame_result* fr);

// msgs / nmsgs / max_frame: the host message table of grdma_h2_pipe_create; reply: the framing stage of
// grdma_h2_pipe_create_reply instead
static grdma_h2_pipe* h2_pipe_create(grdma_stream_job* job, uint32_t link, const grdma_h2_msg* msgs, uint64_t nmsgs,
                                     uint32_t max_frame, grdma_h2_parser* parser, uint64_t delivered_slices,
                                     uint64_t events_cap, grdma_h2_reply* reply, uint64_t recorded_wire_bytes) {
  if (grdma_device_count() <= 0 || !job || !parser) return nullptr;
  if (!reply && (!msgs || !nmsgs || max_frame == 0 || max_frame >= (1u << 24))) return nullptr;
  if (!g_pipe_frame_stream &&
      (hipStreamCreateWithFlags(&g_pipe_frame_stream, hipStreamNonBlocking) != hipSuccess ||
       hipStreamCreateWithFlags(&g_pipe_deframe_stream, hipStreamNonBlocking) != hipSuccess))
    return nullptr;
  grdma_h2_pipe* p = new grdma_h2_pipe();
  p->job = job;
  p->parser = parser;
  p->nmsgs = nmsgs;
  p->max_frame = max_frame;
  p->delivered = delivered_slices;
  p->ev_cap = events_cap;
  p->frame_stream = g_pipe_frame_stream;      // shared by all pipes: framings are ordered among themselves
  p->deframe_stream = g_pipe_deframe_stream;  // shared: the parser state is handed from one deframing to the next
  std::vector<grdma_h2_msg_dev> tmp(nmsgs);
  for (uint64_t i = 0; i < nmsgs; i++) {
    tmp[i].payload = static_cast<const uint8_t*>(msgs[i].payload);
    tmp[i].len = msgs[i].len;
    tmp[i].stream_id = msgs[i].stream_id;
    tmp[i].flags = msgs[i].flags;
  }
  bool ok = grdma_job_link_view(job, link, &p->d_sges, &p->count, &p->d_slices, &p->dst, &p->job_stream) == 0;
  // The deframing goes behind the job on the JOB's stream unless GRDMA_H2_DEFRAME_STREAM=1 asks for a stream of its
  // own: the next job does not start before the deframing has ended either way (measured: kernels of the two streams
  // do not run side by side), and a hand-over between streams costs ~20 us of idle device on each side of it.
  static const bool own_stream = [] { const char* e = getenv("GRDMA_H2_DEFRAME_STREAM"); return e && atoi(e) != 0; }();
  if (ok && !own_stream) p->deframe_stream = p->job_stream;
  p->hdr_cap = 32 * (p->count + 64);
  // (a reply pipe has no message table of its own: the reply's plan builds one per step)
  ok = ok && (reply || (hipMalloc((void**)&p->d_msgs, sizeof(grdma_h2_msg_dev) * nmsgs) == hipSuccess &&
                       hipMalloc((void**)&p->d_pos, sizeof(grdma_h2_msg_pos) * nmsgs) == hipSuccess &&
                       hipMemcpy(p->d_msgs, tmp.data(), sizeof(grdma_h2_msg_dev) * nmsgs, hipMemcpyHostToDevice) == hipSuccess)) &&
       hipMalloc((void**)&p->d_hdr, p->hdr_cap) == hipSuccess &&
       hipMalloc((void**)&p->d_fres, sizeof(grdma_h2_frame_result)) == hipSuccess &&
       hipMalloc((void**)&p->d_dres, sizeof(grdma_h2_deframe_result)) == hipSuccess &&
       hipMalloc((void**)&p->d_ev, sizeof(grdma_h2_event) * (events_cap ? events_cap : 1)) == hipSuccess &&
       hipEventCreateWithFlags(&p->framed, hipEventDisableTiming) == hipSuccess &&
       hipEventCreateWithFlags(&p->job_done, hipEventDisableTiming) == hipSuccess &&
       hipEventCreateWithFlags(&p->deframed, hipEventDisableTiming) == hipSuccess &&
       hipEventCreate(&p->t_f0) == hipSuccess && hipEventCreate(&p->t_f1) == hipSuccess &&
       hipEventCreate(&p->t_d0) == hipSuccess && hipEventCreate(&p->t_d1) == hipSuccess;
  ok = ok && (!reply || h2_reply_bind_pipe(reply, p, recorded_wire_bytes));
  if (!ok) {
    grdma_h2_pipe_destroy(p);
    return nullptr;
  }
  p->chunked = delivered_slices >= H2_CHUNK_MIN_SLICES && h2_chunks_prepare(parser, events_cap, p->deframe_stream);
  // Framing and deframing as nodes of the job's own graph (default; GRDMA_H2_PIPE_FUSED=0: stages enqueued around the
  // graph launch, with per-stage event timing): a graph boundary costs ~15-20 us of idle device on each side.
  const char* fe = getenv("GRDMA_H2_PIPE_FUSED");
  if (!fe || atoi(fe) != 0) {
    auto arg = [](uint64_t v) { return v; };
    auto ptr = [](const void* q) { return (uint64_t)(uintptr_t)q; };
    grdma_job_hook pre[2], post[2];
    memset(pre, 0, sizeof(pre));
    memset(post, 0, sizeof(post));
    const uint64_t per = H2_EMIT_THREADS / 64;
    uint32_t n_pre = 2;
    if (p->reply) {
      n_pre = h2_reply_hooks(p->reply, pre);
    } else if (p->nmsgs <= H2_FRAME_ONE_MAX) {
      pre[0] = grdma_job_hook{(const void*)k_h2_frame_one, (uint32_t)((p->nmsgs + per - 1) / per), H2_EMIT_THREADS,
                              {ptr(p->d_msgs), arg(p->nmsgs), arg(p->max_frame), ptr(p->d_sges), arg(p->count), ptr(p->d_hdr),
                               arg(p->hdr_cap), ptr(p->d_fres)}};
      n_pre = 1;
    } else {
      pre[0] = grdma_job_hook{(const void*)k_h2_frame_index, 1, 256,
                              {ptr(p->d_msgs), arg(p->nmsgs), arg(p->max_frame), arg(p->count), arg(p->hdr_cap), ptr(p->d_pos),
                               ptr(p->d_fres)}};
      pre[1] = grdma_job_hook{(const void*)k_h2_frame_emit, (uint32_t)((p->nmsgs + per - 1) / per), H2_EMIT_THREADS,
                              {ptr(p->d_msgs), arg(p->nmsgs), arg(p->max_frame), ptr(p->d_sges), arg(p->count), ptr(p->d_hdr),
                               arg(p->hdr_cap), ptr(p->d_pos)}};
    }
    uint32_t n_post;
    if (p->chunked) {
      post[0] = grdma_job_hook{(const void*)k_h2_deframe_chunks, (uint32_t)parser->chunks_want, H2_DEFRAME_THREADS,
                               {ptr(parser->d), ptr(parser->d_chunks), ptr(p->dst), ptr(p->d_slices), arg(p->delivered)}};
      post[1] = grdma_job_hook{(const void*)k_h2_merge_or_deframe, H2_MERGE_GRID, H2_DEFRAME_THREADS,
                               {ptr(parser->d), ptr(parser->d_chunks), ptr(p->dst), ptr(p->d_slices), arg(p->delivered),
                                ptr(p->d_ev), arg(p->ev_cap), ptr(p->d_dres)}};
      n_post = 2;
    } else {
      post[0] = grdma_job_hook{(const void*)k_h2_deframe, 1, H2_DEFRAME_THREADS,
                               {ptr(parser->d), ptr(p->dst), ptr(p->d_slices), arg(p->delivered), ptr(p->d_ev), arg(p->ev_cap),
                                ptr(p->d_dres)}};
      n_post = 1;
    }
    memcpy(p->pre, pre, sizeof(pre));
    memcpy(p->post, post, sizeof(post));
    p->n_pre = n_pre;
    p->n_post = n_post;
    if (grdma_job_set_hooks(job, pre, n_pre, post, n_post) != 0) {
      grdma_h2_pipe_destroy(p);
      return nullptr;
    }
    p->fused = true;
    p->deframe_stream = p->job_stream;
  }
  return p;
}

grdma_h2_pipe* grdma_h2_pipe_create(grdma_stream_job* job, uint32_t link, const grdma_h2_msg* msgs, uint64_t nmsgs,
                                    uint32_t max_frame, grdma_h2_parser* parser, uint64_t delivered_slices,
                                    uint64_t events_cap) {
  return h2_pipe_create(job, link, msgs, nmsgs, max_frame, parser, delivered_slices, events_cap, nullptr, 0);
}

grdma_h2_pipe* grdma_h2_pipe_create_reply(grdma_stream_job* job_back, uint32_t link, grdma_h2_reply* reply,
                                          grdma_h2_parser* parser_back, uint64_t delivered_slices, uint64_t events_cap,
                                          uint64_t recorded_wire_bytes) {
  if (!reply) return nullptr;
  return h2_pipe_create(job_back, link, nullptr, 0, 0, parser_back, delivered_slices, events_cap, reply, recorded_wire_bytes);
}

void grdma_h2_pipe_destroy(grdma_h2_pipe* p) {
  if (!p) return;
  if (h2_asm_read_by_reply_pipes(p->asm_)) return;  // (a reply pipe's job gathers from this pipe's arena: destroy that one first)
  if (p->launched) {
    hipStreamSynchronize(p->frame_stream);
    hipStreamSynchronize(p->job_stream);
    hipStreamSynchronize(p->deframe_stream);
  }
  if (p->parser && p->parser->last_deframed == p->deframed) p->parser->last_deframed = nullptr;  // (synchronised above)
  if (p->fused && p->job) grdma_job_set_hooks(p->job, nullptr, 0, nullptr, 0);
  h2_reply_unbind_pipe(p);
  h2_asm_detach(p);
  hipFree(p->d_call);
  hipFree(p->d_msgs);
  hipFree(p->d_pos);
  hipFree(p->d_hdr);
  hipFree(p->d_fres);
  hipFree(p->d_dres);
  hipFree(p->d_ev);
  if (p->framed) hipEventDestroy(p->framed);
  if (p->job_done) hipEventDestroy(p->job_done);
  if (p->deframed) hipEventDestroy(p->deframed);
  for (hipEvent_t e : {p->t_f0, p->t_f1, p->t_d0, p->t_d1})
    if (e) hipEventDestroy(e);
  delete p;
}

// One step on the job's captured graph (schedule 0: the only schedule since the link engine was retired).
int grdma_h2_pipe_enqueue(grdma_h2_pipe* p, int schedule) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || schedule != 0) return -GRDMA_ERR_INVALID;
  if (p->fused && schedule == 0) {
    // one graph launch: [k_h2_frame_index, k_h2_frame_emit] -> the job's rounds -> [the deframer]; steps and pipes
    // of one connection are ordered by the job's stream (a parser last used on another stream: by its event)
    if (p->parser->last_deframed && p->parser->last_stream != p->job_stream &&
        hipStreamWaitEvent(p->job_stream, p->parser->last_deframed, 0) != hipSuccess)
      return -GRDMA_ERR_HIP;
    // a reply step reads what the forward step assembled; a forward step's release waits for the reply step that
    // still gathers from the arena
    if (p->reply && h2_reply_wait_source(p, p->job_stream) != 0) return -GRDMA_ERR_HIP;
    if (hipEvent_t rd = h2_asm_last_read(p->asm_))
      if (hipStreamWaitEvent(p->job_stream, rd, 0) != hipSuccess) return -GRDMA_ERR_HIP;
    const int rc = grdma_stream_job_launch(p->job);
    if (rc < 0) return rc;
    if (hipEventRecord(p->deframed, p->job_stream) != hipSuccess) return -GRDMA_ERR_HIP;
    if (p->reply) h2_reply_step_enqueued(p, p->deframed);
    p->parser->last_stream = p->job_stream;
    p->parser->last_deframed = p->deframed;
    p->launched = true;
    p->timed = false;
    return 0;
  }
  p->timed = true;
  // framing overwrites the slice table the job's previous step read
  if (p->launched && hipStreamWaitEvent(p->frame_stream, p->job_done, 0) != hipSuccess) return -GRDMA_ERR_HIP;
  if (hipMemsetAsync(p->d_fres, 0, sizeof(grdma_h2_frame_result), p->frame_stream) != hipSuccess) return -GRDMA_ERR_HIP;
  if (p->reply && h2_reply_wait_source(p, p->frame_stream) != 0) return -GRDMA_ERR_HIP;
  hipEventRecord(p->t_f0, p->frame_stream);
  if (p->reply)
    h2_reply_enqueue(p->reply, p->frame_stream);
  else
    h2_enqueue_frame(p->d_msgs, p->nmsgs, p->max_frame, p->d_sges, p->count, p->d_hdr, p->hdr_cap, p->d_pos, p->d_fres,
                     p->frame_stream);
  hipEventRecord(p->t_f1, p->frame_stream);
  if (hipEventRecord(p->framed, p->frame_stream) != hipSuccess) return -GRDMA_ERR_HIP;
  // the job reads the slice table and overwrites what the previous deframing parsed
  if (hipStreamWaitEvent(p->job_stream, p->framed, 0) != hipSuccess) return -GRDMA_ERR_HIP;
  if (p->launched && p->deframe_stream != p->job_stream && hipStreamWaitEvent(p->job_stream, p->deframed, 0) != hipSuccess)
    return -GRDMA_ERR_HIP;
  const int rc = grdma_stream_job_launch(p->job);
  if (rc < 0) return rc;
  if (hipEventRecord(p->job_done, p->job_stream) != hipSuccess) return -GRDMA_ERR_HIP;
  if (p->reply) h2_reply_step_enqueued(p, p->job_done);
  if (p->deframe_stream != p->job_stream && hipStreamWaitEvent(p->deframe_stream, p->job_done, 0) != hipSuccess)
    return -GRDMA_ERR_HIP;
  if (p->parser->last_deframed && p->parser->last_stream != p->deframe_stream &&
      hipStreamWaitEvent(p->deframe_stream, p->parser->last_deframed, 0) != hipSuccess)
    return -GRDMA_ERR_HIP;  // (the parser state is handed from one deframing to the next)
  hipEventRecord(p->t_d0, p->deframe_stream);
  h2_enqueue_deframe(p->parser, p->dst, p->d_slices, p->delivered, p->d_ev, p->ev_cap, p->d_dres, p->deframe_stream, p->chunked);
  if (hipEvent_t rd = h2_asm_last_read(p->asm_))  // (the release at the start of the assembly, behind the reply's gather)
    if (hipStreamWaitEvent(p->deframe_stream, rd, 0) != hipSuccess) return -GRDMA_ERR_HIP;
  if (p->asm_) h2_asm_enqueue(p->asm_, p->d_call, p->deframe_stream);
  hipEventRecord(p->t_d1, p->deframe_stream);
  if (hipEventRecord(p->deframed, p->deframe_stream) != hipSuccess) return -GRDMA_ERR_HIP;
  p->parser->last_stream = p->deframe_stream;
  p->parser->last_deframed = p->deframed;
  p->launched = true;
  return 0;
}

// Wait for the last step and report it: out = {slices framed, frame overflow, events, deframe
// overflow, slices parsed, h2 error, framing kernel us, deframing kernel us, bulk steps, frames
// parsed by bulk steps, then the deframer's device-clock ticks: waiting for the look-ahead ring,
// in bulk steps, total, in the byte-wise path}; events_out (may be NULL) receives up to cap events.
int grdma_h2_pipe_sync(grdma_h2_pipe* p, uint64_t out[14], grdma_h2_event* events_out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !out) return -GRDMA_ERR_INVALID;
  if (hipStreamSynchronize(p->frame_stream) != hipSuccess || hipStreamSynchronize(p->job_stream) != hipSuccess ||
      hipStreamSynchronize(p->deframe_stream) != hipSuccess)
    return -GRDMA_ERR_HIP;
  grdma_h2_frame_result fr;
  grdma_h2_deframe_result dr;
  if (hipMemcpy(&fr, p->d_fres, sizeof(fr), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&dr, p->d_dres, sizeof(dr), hipMemcpyDeviceToHost) != hipSuccess)
    return -GRDMA_ERR_HIP;
  if (p->reply && !h2_reply_result(p->reply, &fr)) return -GRDMA_ERR_HIP;  // (overflow 2: not the recorded shape)
  out[0] = fr.nslices;
  out[1] = fr.overflow;
  out[2] = dr.nevents;
  out[3] = dr.overflow;
  out[4] = dr.slices_done;
  out[5] = (uint64_t)dr.error;
  out[8] = dr.bulk_steps;
  out[9] = dr.bulk_frames;
  out[10] = dr.t_wait;
  out[11] = dr.t_bulk;
  out[12] = dr.t_total;
  out[13] = dr.t_serial;
  p->boundary_steps = dr.boundary_steps;
  p->t_boundary = dr.t_boundary;
  float fms = 0, dms = 0;
  out[6] = out[7] = 0;
  if (p->launched && p->timed && hipEventElapsedTime(&fms, p->t_f0, p->t_f1) == hipSuccess) out[6] = (uint64_t)(fms * 1e3f);
  if (p->launched && p->timed && hipEventElapsedTime(&dms, p->t_d0, p->t_d1) == hipSuccess) out[7] = (uint64_t)(dms * 1e3f);
  const uint64_t m = std::min<uint64_t>(std::min<uint64_t>(dr.nevents, cap), p->ev_cap);
  if (events_out && m && hipMemcpy(events_out, p->d_ev, sizeof(grdma_h2_event) * m, hipMemcpyDeviceToHost) != hipSuccess)
    return -GRDMA_ERR_HIP;
  return 0;
}


// {message starts taken by the boundary step, device-clock ticks inside it} of the last synced step
int grdma_h2_pipe_boundary_stats(grdma_h2_pipe* p, uint64_t out[2]) {
  if (!p || !out) return -GRDMA_ERR_INVALID;
  out[0] = p->boundary_steps;
  out[1] = p->t_boundary;
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

// the assembly of one call, enqueued on st behind its deframing
static void h2_asm_enqueue(grdma_h2_asm* a, const h2a_call* d_call, hipStream_t st) {
  h2a_dev* d = a->d;
  hipLaunchKernelGGL(k_h2_asm_tiles, dim3(H2A_GRID), dim3(H2A_THREADS), 0, st, d, d_call);
  hipLaunchKernelGGL(k_h2_asm_carry, dim3(1), dim3(H2A_ONE_THREADS), 0, st, d, d_call);
  hipLaunchKernelGGL(k_h2_asm_begin, dim3(H2A_GRID), dim3(H2A_THREADS), 0, st, d, d_call);
  hipLaunchKernelGGL(k_h2_asm_bytes, dim3(H2A_GRID), dim3(H2A_THREADS), 0, st, d, d_call);
  hipLaunchKernelGGL(k_h2_asm_finish, dim3(1), dim3(H2A_ONE_THREADS), 0, st, d, d_call);
  hipLaunchKernelGGL(k_h2_asm_copy, dim3(H2A_GRID), dim3(H2A_THREADS), 0, st, d, d_call);
}

// the same six kernels as post hooks of a fused pipe's graph, behind the deframer's
static uint32_t h2_asm_hooks(grdma_h2_asm* a, const h2a_call* d_call, grdma_job_hook* out) {
  const void* fns[6] = {(const void*)k_h2_asm_tiles, (const void*)k_h2_asm_carry, (const void*)k_h2_asm_begin,
                        (const void*)k_h2_asm_bytes, (const void*)k_h2_asm_finish, (const void*)k_h2_asm_copy};
  const uint32_t grids[6] = {H2A_GRID, 1, H2A_GRID, H2A_GRID, 1, H2A_GRID};
  const uint32_t threads[6] = {H2A_THREADS, H2A_ONE_THREADS, H2A_THREADS, H2A_THREADS, H2A_ONE_THREADS, H2A_THREADS};
  for (int k = 0; k < 6; k++) {
    memset(&out[k], 0, sizeof(out[k]));
    out[k].fn = fns[k];
    out[k].grid = grids[k];
    out[k].threads = threads[k];
    out[k].args[0] = (uint64_t)(uintptr_t)a->d;
    out[k].args[1] = (uint64_t)(uintptr_t)d_call;
  }
  return 6;
}

static void h2_asm_detach(grdma_h2_pipe* p) {
  if (p->asm_) {
    p->asm_->parser->asm_attached--;
    p->asm_->attached--;
    p->asm_ = nullptr;
  }
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
  h2_enqueue_deframe(p, static_cast<const uint8_t*>(d_arena), p->d_sl, n, p->d_ev, ev_cap, p->d_res, st, chunked);
  // the assembly: the plan (five kernels), then the copy, timed apart
  h2a_dev* d = a->d;
  hipEventRecord(a->e0, st);
  hipLaunchKernelGGL(k_h2_asm_tiles, dim3(H2A_GRID), dim3(H2A_THREADS), 0, st, d, (const h2a_call*)a->d_call);
  hipLaunchKernelGGL(k_h2_asm_carry, dim3(1), dim3(H2A_ONE_THREADS), 0, st, d, (const h2a_call*)a->d_call);
  hipLaunchKernelGGL(k_h2_asm_begin, dim3(H2A_GRID), dim3(H2A_THREADS), 0, st, d, (const h2a_call*)a->d_call);
  hipLaunchKernelGGL(k_h2_asm_bytes, dim3(H2A_GRID), dim3(H2A_THREADS), 0, st, d, (const h2a_call*)a->d_call);
  hipLaunchKernelGGL(k_h2_asm_finish, dim3(1), dim3(H2A_ONE_THREADS), 0, st, d, (const h2a_call*)a->d_call);
  hipEventRecord(a->e1, st);
  hipLaunchKernelGGL(k_h2_asm_copy, dim3(H2A_GRID), dim3(H2A_THREADS), 0, st, d, (const h2a_call*)a->d_call);
  hipEventRecord(a->e2, st);
  grdma_h2_deframe_result h_res;
  h2a_dev h;
  if (hipMemcpyAsync(&h_res, p->d_res, sizeof(h_res), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  if (hipEventElapsedTime(&a->plan_ms, a->e0, a->e1) != hipSuccess) a->plan_ms = 0;
  if (hipEventElapsedTime(&a->copy_ms, a->e1, a->e2) != hipSuccess) a->copy_ms = 0;
  if (h2_error) *h2_error = (int)h_res.error;
  const uint64_t m = h_res.nevents < ev_cap ? h_res.nevents : ev_cap;
  if (events_out && m &&
      (hipMemcpyAsync(events_out, p->d_ev, sizeof(grdma_h2_event) * m, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipStreamSynchronize(st) != hipSuccess))
    return -GRDMA_ERR_HIP;
  if (h_res.overflow || h.skip) return -GRDMA_ERR_CAPACITY;
  if (h.ndesc > msgs_cap || h.ndesc > h.desc_cap) return -GRDMA_ERR_CAPACITY;
  if (h.ndesc && (hipMemcpyAsync(msgs_out, h.desc, sizeof(grdma_h2_rx_msg) * h.ndesc, hipMemcpyDeviceToHost, st) != hipSuccess ||
                  hipStreamSynchronize(st) != hipSuccess))
    return -GRDMA_ERR_HIP;
  return (int64_t)h.ndesc;
}

int grdma_h2_asm_release(grdma_h2_asm* a, uint64_t count) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!a || a->attached) return -GRDMA_ERR_INVALID;  // (a pipe step releases everything reported before it itself)
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  // behind the last standalone call (same stream) and the last pipe step of the parser
  if (a->parser->last_deframed && hipStreamWaitEvent(hc->stream, a->parser->last_deframed, 0) != hipSuccess)
    return -GRDMA_ERR_HIP;
  hipLaunchKernelGGL(k_h2_asm_release, dim3(1), dim3(64), 0, hc->stream, a->d, count);
  return hipGetLastError() == hipSuccess ? 0 : -GRDMA_ERR_HIP;
}

int grdma_h2_asm_stats(grdma_h2_asm* a, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!a || !out) return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  h2a_dev h;
  if (a->parser->last_deframed && hipStreamWaitEvent(hc->stream, a->parser->last_deframed, 0) != hipSuccess)
    return -GRDMA_ERR_HIP;
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

int grdma_h2_pipe_attach_assembler(grdma_h2_pipe* p, grdma_h2_asm* a) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !a || a->parser != p->parser || p->asm_) return -GRDMA_ERR_INVALID;
  if (p->launched && hipStreamSynchronize(p->deframe_stream) != hipSuccess) return -GRDMA_ERR_HIP;
  if (!h2_asm_prepare(a, p->ev_cap ? p->ev_cap : 1)) return -GRDMA_ERR_HIP;
  const h2a_call call{p->d_ev, p->d_dres, p->d_slices, p->dst, p->ev_cap, 1};
  if (!p->d_call && hipMalloc((void**)&p->d_call, sizeof(h2a_call)) != hipSuccess) return -GRDMA_ERR_HIP;
  if (hipMemcpy(p->d_call, &call, sizeof(call), hipMemcpyHostToDevice) != hipSuccess) return -GRDMA_ERR_HIP;
  if (p->fused) {
    grdma_job_hook post[8];
    memcpy(post, p->post, sizeof(grdma_job_hook) * p->n_post);
    const uint32_t n_post = p->n_post + h2_asm_hooks(a, p->d_call, post + p->n_post);
    if (grdma_job_set_hooks(p->job, p->pre, p->n_pre, post, n_post) != 0) return -GRDMA_ERR_HIP;
  }
  p->asm_ = a;
  a->attached++;
  a->parser->asm_attached++;
  return 0;
}

int64_t grdma_h2_pipe_messages(grdma_h2_pipe* p, grdma_h2_rx_msg* out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !p->asm_ || (!out && cap)) return -GRDMA_ERR_INVALID;
  h2a_dev h;
  // the step's assembly ends with its deframing event (fused: the job's graph; else the deframe stream)
  if ((p->launched && hipEventSynchronize(p->deframed) != hipSuccess) || hipStreamSynchronize(p->deframe_stream) != hipSuccess ||
      hipMemcpy(&h, p->asm_->d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)
    return -GRDMA_ERR_HIP;
  if (h.skip || h.ndesc > cap || h.ndesc > h.desc_cap) return -GRDMA_ERR_CAPACITY;
  if (h.ndesc && hipMemcpy(out, h.desc, sizeof(grdma_h2_rx_msg) * h.ndesc, hipMemcpyDeviceToHost) != hipSuccess)
    return -GRDMA_ERR_HIP;
  return (int64_t)h.ndesc;
}

// ---- replies framed from the descriptors (csrc/grdma_h2_reply.h) ---------------------------------------------
struct grdma_h2_group_pipe;
struct grdma_h2_reply {
  grdma_h2_asm* src = nullptr;
  h2r_dev* d = nullptr;
  h2r_dev h;                        // host copy of the configuration words
  grdma_h2_route* d_routes = nullptr;
  grdma_h2_pipe* pipe = nullptr;    // the reply pipe that frames through it (at most one: the scratch is one call's)
  grdma_h2_group_pipe* gpipe = nullptr;  // ... or the group reply pipe (grdma_h2_group_pipe_create_reply)
  hipEvent_t e0 = nullptr, e1 = nullptr;
};

static void h2_reply_enqueue(grdma_h2_reply* r, hipStream_t st) {
  hipLaunchKernelGGL(k_h2_reply_plan, dim3(1), dim3(PLAN_THREADS), 0, st, r->d);
  hipLaunchKernelGGL(k_h2_reply_emit, dim3(H2R_GRID), dim3(H2_EMIT_THREADS), 0, st, (const h2r_dev*)r->d);
}

// the same two kernels as pre hooks of the back job's graph: a linear chain in front of its first round
static uint32_t h2_reply_hooks(grdma_h2_reply* r, grdma_job_hook* out) {
  memset(out, 0, 2 * sizeof(grdma_job_hook));
  out[0].fn = (const void*)k_h2_reply_plan;
  out[0].grid = 1;
  out[0].threads = PLAN_THREADS;
  out[1].fn = (const void*)k_h2_reply_emit;
  out[1].grid = H2R_GRID;
  out[1].threads = H2_EMIT_THREADS;
  out[0].args[0] = out[1].args[0] = (uint64_t)(uintptr_t)r->d;
  return 2;
}

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

static bool h2_reply_bind_pipe(grdma_h2_reply* r, grdma_h2_pipe* p, uint64_t recorded_wire_bytes) {
  if (r->pipe || r->gpipe || !r->src->attached) return false;  // (the source of a reply pipe assembles in forward pipes)
  if (!h2_reply_set_target(r, p->d_sges, p->count, p->d_hdr, p->hdr_cap, 1, p->count, recorded_wire_bytes, nullptr)) return false;
  r->pipe = p;
  r->src->reply_pipes++;
  p->reply = r;
  p->max_frame = r->h.max_frame;
  return true;
}

static void h2_reply_unbind_pipe(grdma_h2_pipe* p) {
  grdma_h2_reply* r = p->reply;
  if (!r) return;
  // (the pipe's streams are synchronised: nothing gathers from the source's arena any more)
  if (r->src->last_read == p->deframed || r->src->last_read == p->job_done) r->src->last_read = nullptr;
  r->src->reply_pipes--;
  r->pipe = nullptr;
  p->reply = nullptr;
}

static bool h2_asm_read_by_reply_pipes(const grdma_h2_asm* a) { return a && a->reply_pipes != 0; }
static hipEvent_t h2_asm_last_read(const grdma_h2_asm* a) { return a ? a->last_read : nullptr; }

// the reply's plan goes behind the assembly of the last forward step enqueued (the forward parser's event)
static int h2_reply_wait_source(grdma_h2_pipe* p, hipStream_t st) {
  const grdma_h2_parser* fp = p->reply->src->parser;
  if (fp->last_deframed && fp->last_stream != st && hipStreamWaitEvent(st, fp->last_deframed, 0) != hipSuccess) return -1;
  return 0;
}

static void h2_reply_step_enqueued(grdma_h2_pipe* p, hipEvent_t read_done) { p->reply->src->last_read = read_done; }

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
  if (!r || r->pipe || r->gpipe) return;  // (the pipe's graph still runs the kernels on it: destroy the pipe first)
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
      ((uintptr_t)d_hdr_arena & 15) || r->pipe || r->gpipe || r->src->attached)
    return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  // the stream of grdma_h2_deframe_messages: the call is ordered behind the one it reads
  hipStream_t st = hc->stream;
  if (!h2_reply_set_target(r, reinterpret_cast<grdma_sge*>(d_slices_out), slices_cap, static_cast<uint8_t*>(d_hdr_arena),
                           hdr_cap, 0, 0, 0, st))
    return -GRDMA_ERR_HIP;
  hipEventRecord(r->e0, st);
  h2_reply_enqueue(r, st);
  hipEventRecord(r->e1, st);
  uint64_t res[8];
  if (hipMemcpyAsync(res, reinterpret_cast<uint8_t*>(r->d) + offsetof(h2r_dev, res), sizeof(res), hipMemcpyDeviceToHost, st) !=
          hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  float ms = 0;
  for (int i = 0; i < 7; i++) out[i] = res[i];
  out[7] = hipEventElapsedTime(&ms, r->e0, r->e1) == hipSuccess ? (uint64_t)(ms * 1e3f) : 0;
  if (res[H2R_OVERFLOW]) return -GRDMA_ERR_CAPACITY;
  return (int64_t)res[H2R_SLICES];
}

// ---- the replies of many transports in two launches (k_h2_reply_plan_links, k_h2_reply_emit_links) ----------------
// The batch block of the process holds the call: [table | one h2r_dev per item] goes up in one copy -- the item's
// framer with the item's targets and a zeroed result block; scratch, routes and source stay the reply's own -- and the
// h2r_dev blocks come down in one copy.  One call at a time, as the other batch calls.
static_assert(H2R_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the reply's link table is the batch's");

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
    if (it.reply->pipe || it.reply->gpipe) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 reply batch: a reply bound to a reply pipe");
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
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_parser* p = items[i].reply->src->parser;
    if (p->last_deframed && p->last_stream != st && hipStreamWaitEvent(st, p->last_deframed, 0) != hipSuccess) return -GRDMA_ERR_HIP;
  }
  if (hipMemcpyAsync(d, up.data(), total, hipMemcpyHostToDevice, st) != hipSuccess) return -GRDMA_ERR_HIP;
  hipEventRecord(hc->e0, st);
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_h2_reply_plan_links, dim3(n_items), dim3(PLAN_THREADS), 0, st, (const h2r_link*)d);
  hipLaunchKernelGGL(k_h2_reply_emit_links, dim3(H2R_GRID), dim3(H2_EMIT_THREADS), 0, st, (const h2r_link*)d, n_items);
  if (hipGetLastError() != hipSuccess) {
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

int64_t grdma_h2_pipe_slice_table(grdma_h2_pipe* p, grdma_slice* out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || (!out && cap)) return -GRDMA_ERR_INVALID;
  if (p->count > cap) return -GRDMA_ERR_CAPACITY;
  static_assert(sizeof(grdma_slice) == sizeof(grdma_sge), "layout");
  if (hipStreamSynchronize(p->frame_stream) != hipSuccess || hipStreamSynchronize(p->job_stream) != hipSuccess ||
      (p->count && hipMemcpy(out, p->d_sges, sizeof(grdma_sge) * p->count, hipMemcpyDeviceToHost) != hipSuccess))
    return -GRDMA_ERR_HIP;
  return (int64_t)p->count;
}

// ---- HTTP/2 on several links of ONE job (the group pipe) -----------------------------------------------------------
// A job carries one set of hooks (grdma_job_set_hooks assigns): the stages of all listed links are ONE framing kernel
// over a table of links (k_h2_frame_links) in front of the job and ONE deframing kernel (k_h2_deframe_links) behind
// it -- one launch per step however many links.  Links that are not listed keep their tables and are carried as before.
struct h2_group_link {
  uint32_t link = 0;
  grdma_h2_parser* parser = nullptr;
  grdma_sge* d_sges = nullptr;
  uint64_t count = 0;
  grdma_slice_out* d_slices = nullptr;
  uint8_t* dst = nullptr;
  grdma_h2_msg_dev* d_msgs = nullptr;
  uint64_t nmsgs = 0;
  uint8_t* d_hdr = nullptr;
  uint64_t hdr_cap = 0;
  grdma_h2_event* d_ev = nullptr;
  uint64_t ev_cap = 0, delivered = 0;
};
struct grdma_h2_group_pipe {
  grdma_stream_job* job = nullptr;
  std::vector<h2_group_link> links;
  hipStream_t job_stream = nullptr, frame_stream = nullptr;
  grdma_h2_link_frame* d_ftab = nullptr;
  grdma_h2_link_deframe* d_dtab = nullptr;
  grdma_h2_frame_result* d_fres = nullptr;    // one per listed link
  grdma_h2_deframe_result* d_dres = nullptr;  // one per listed link
  uint32_t frame_grid = 0;
  hipEvent_t framed = nullptr, job_done = nullptr, deframed = nullptr;
  hipEvent_t t_f0 = nullptr, t_f1 = nullptr, t_d0 = nullptr, t_d1 = nullptr;
  bool launched = false, fused = false, timed = false;
  grdma_job_hook pre[2], post;        // the framing kernel(s) and the deframing kernel in the job's graph (fused)
  uint32_t n_pre = 0;
  // a group reply pipe (grdma_h2_group_pipe_create_reply): the framing stage is k_h2_reply_plan_links + k_h2_reply_emit_links
  std::vector<grdma_h2_reply*> replies;  // per spec
  h2r_link* d_rtab = nullptr;
  std::vector<grdma_h2_asm*> asms;    // per spec, NULL = none (grdma_h2_group_pipe_attach_assemblers)
  h2a_link* d_atab = nullptr;         // the links with an assembler, in spec order
  h2a_call* d_calls = nullptr;        // their call blocks
  uint32_t n_asm = 0;
};
static void h2_asm_links_enqueue(const h2a_link* d_tab, uint32_t n, hipStream_t st);
static void h2_group_detach(grdma_h2_group_pipe* p);
static void h2_group_unbind_replies(grdma_h2_group_pipe* p);

static grdma_h2_group_pipe* h2_group_refuse(grdma_h2_group_pipe* p, const char* why) {
  grdma_h2_group_pipe_destroy(p);
  grdma_fail_msg(GRDMA_ERR_INVALID, why);
  return nullptr;
}

// specs: the message tables of grdma_h2_group_pipe_create; rspecs: the replies of grdma_h2_group_pipe_create_reply
// instead (exactly one of the two)
static grdma_h2_group_pipe* h2_group_create(grdma_stream_job* job, const grdma_h2_link_spec* specs,
                                            const grdma_h2_reply_link_spec* rspecs, uint32_t n, uint32_t max_frame) {
  if (grdma_device_count() <= 0) return nullptr;
  if (!job || (!specs && !rspecs) || n == 0 || n > GRDMA_H2_BATCH_MAX) return h2_group_refuse(nullptr, "h2 group pipe: a job and 1 .. GRDMA_H2_BATCH_MAX link specs");
  if (specs && (max_frame == 0 || max_frame >= (1u << 24))) return h2_group_refuse(nullptr, "h2 group pipe: max_frame out of range");
  auto link_of = [&](uint32_t i) { return specs ? specs[i].link : rspecs[i].link; };
  auto parser_of = [&](uint32_t i) { return specs ? specs[i].parser : rspecs[i].parser_back; };
  for (uint32_t i = 0; i < n; i++) {
    if (specs && (!specs[i].msgs || specs[i].nmsgs == 0 || specs[i].nmsgs > H2_FRAME_ONE_MAX))
      return h2_group_refuse(nullptr, "h2 group pipe: 1 .. 4096 messages per link");
    if (rspecs && !rspecs[i].reply) return h2_group_refuse(nullptr, "h2 group reply pipe: a link without reply");
    if (!parser_of(i)) return h2_group_refuse(nullptr, "h2 group pipe: a link without parser");
    for (uint32_t k = 0; k < i; k++) {
      if (link_of(k) == link_of(i)) return h2_group_refuse(nullptr, "h2 group pipe: a link listed twice");
      if (parser_of(k) == parser_of(i)) return h2_group_refuse(nullptr, "h2 group pipe: a parser listed twice");
      if (rspecs && rspecs[k].reply == rspecs[i].reply) return h2_group_refuse(nullptr, "h2 group reply pipe: a reply listed twice");
    }
  }
  const uint32_t job_links = grdma_job_link_count(job);
  for (uint32_t i = 0; i < n; i++)
    if (link_of(i) >= job_links) return h2_group_refuse(nullptr, "h2 group pipe: a link index out of range");
  for (uint32_t i = 0; specs && i < n; i++)
    for (uint64_t k = 0; k < specs[i].nmsgs; k++)
      if (specs[i].msgs[k].len >= (1ull << 32)) return h2_group_refuse(nullptr, "h2 group pipe: a message of 4 GiB or more");
  for (uint32_t i = 0; rspecs && i < n; i++) {
    const grdma_h2_reply* r = rspecs[i].reply;
    if (r->pipe || r->gpipe) return h2_group_refuse(nullptr, "h2 group reply pipe: a reply bound to a pipe already");
    // (the source of a reply pipe assembles in forward pipes: a standalone source is framed by grdma_h2_reply_frame)
    if (!r->src->attached) return h2_group_refuse(nullptr, "h2 group reply pipe: a source assembler that is not attached to a forward pipe");
  }
  uint32_t have[2] = {0, 0};
  if (grdma_job_hook_counts(job, have) != 0) return nullptr;
  if (have[0] || have[1]) return h2_group_refuse(nullptr, "h2 group pipe: the job already carries hooks (another pipe's)");
  if (!g_pipe_frame_stream &&
      (hipStreamCreateWithFlags(&g_pipe_frame_stream, hipStreamNonBlocking) != hipSuccess ||
       hipStreamCreateWithFlags(&g_pipe_deframe_stream, hipStreamNonBlocking) != hipSuccess))
    return nullptr;
  grdma_h2_group_pipe* p = new grdma_h2_group_pipe();
  p->job = job;
  p->frame_stream = g_pipe_frame_stream;
  p->links.resize(n);
  std::vector<grdma_h2_link_frame> ftab(n);
  std::vector<grdma_h2_link_deframe> dtab(n);
  const uint64_t per = H2_EMIT_THREADS / 64;
  std::vector<h2r_link> rtab(n);
  bool ok = hipMalloc((void**)&p->d_ftab, sizeof(grdma_h2_link_frame) * n) == hipSuccess &&
            (!rspecs || hipMalloc((void**)&p->d_rtab, sizeof(h2r_link) * n) == hipSuccess) &&
            hipMalloc((void**)&p->d_dtab, sizeof(grdma_h2_link_deframe) * n) == hipSuccess &&
            hipMalloc((void**)&p->d_fres, sizeof(grdma_h2_frame_result) * n) == hipSuccess &&
            hipMalloc((void**)&p->d_dres, sizeof(grdma_h2_deframe_result) * n) == hipSuccess &&
            hipMemset(p->d_fres, 0, sizeof(grdma_h2_frame_result) * n) == hipSuccess &&
            hipMemset(p->d_dres, 0, sizeof(grdma_h2_deframe_result) * n) == hipSuccess;
  for (uint32_t i = 0; ok && i < n; i++) {
    h2_group_link& l = p->links[i];
    const uint64_t* d_step = nullptr;
    uint64_t slices_cap = 0;
    if (grdma_job_link_view(job, link_of(i), &l.d_sges, &l.count, &l.d_slices, &l.dst, &p->job_stream) != 0 ||
        grdma_job_link_step_slices(job, link_of(i), &d_step, &slices_cap) != 0)
      return h2_group_refuse(p, "h2 group pipe: a link index out of range");
    l.link = link_of(i);
    l.parser = parser_of(i);
    l.nmsgs = specs ? specs[i].nmsgs : 0;
    l.delivered = specs ? specs[i].delivered_slices : rspecs[i].delivered_slices;
    l.ev_cap = specs ? specs[i].events_cap : rspecs[i].events_cap;
    l.hdr_cap = 32 * (l.count + 64);
    ok = hipMalloc((void**)&l.d_hdr, l.hdr_cap) == hipSuccess &&
         hipMalloc((void**)&l.d_ev, sizeof(grdma_h2_event) * (l.ev_cap ? l.ev_cap : 1)) == hipSuccess;
    if (specs) {
      const grdma_h2_link_spec& sp = specs[i];
      std::vector<grdma_h2_msg_dev> tmp(sp.nmsgs);
      for (uint64_t k = 0; k < sp.nmsgs; k++) {
        tmp[k].payload = static_cast<const uint8_t*>(sp.msgs[k].payload);
        tmp[k].len = sp.msgs[k].len;
        tmp[k].stream_id = sp.msgs[k].stream_id;
        tmp[k].flags = sp.msgs[k].flags;
      }
      ok = ok && hipMalloc((void**)&l.d_msgs, sizeof(grdma_h2_msg_dev) * sp.nmsgs) == hipSuccess &&
           hipMemcpy(l.d_msgs, tmp.data(), sizeof(grdma_h2_msg_dev) * sp.nmsgs, hipMemcpyHostToDevice) == hipSuccess;
    } else if (ok) {
      // the link's framer writes the link's slice table, and only a reply of the shape the job's graph was recorded for
      grdma_h2_reply* r = rspecs[i].reply;
      ok = h2_reply_set_target(r, l.d_sges, l.count, l.d_hdr, l.hdr_cap, 1, l.count, rspecs[i].recorded_wire_bytes, nullptr);
      if (ok) {
        r->gpipe = p;
        r->src->reply_pipes++;
        p->replies.push_back(r);
        rtab[i].R = r->d;
      }
    }
    grdma_h2_link_frame& f = ftab[i];
    f.msgs = l.d_msgs;
    f.nmsgs = l.nmsgs;
    f.out = l.d_sges;
    f.cap = l.count;
    f.hdr = l.d_hdr;
    f.hdr_cap = l.hdr_cap;
    f.res = p->d_fres + i;
    f.max_frame = max_frame;
    f.wg0 = p->frame_grid;
    p->frame_grid += (uint32_t)((l.nmsgs + per - 1) / per);
    // the step's own slice count, as the job's drain leaves it on the device (the recorded run's count is what the
    // caller expects; a step at another ring phase may deliver a slice more or less), bounded by the table
    grdma_h2_link_deframe& q = dtab[i];
    q.res = p->d_dres + i;
    q.gp = l.parser->d;
    q.arena = l.dst;
    q.slices = l.d_slices;
    q.nslices = slices_cap;
    q.ev = l.d_ev;
    q.ev_cap = l.ev_cap;
    q.n_step = d_step;
  }
  ok = ok && hipMemcpy(p->d_ftab, ftab.data(), sizeof(grdma_h2_link_frame) * n, hipMemcpyHostToDevice) == hipSuccess &&
       (!rspecs || hipMemcpy(p->d_rtab, rtab.data(), sizeof(h2r_link) * n, hipMemcpyHostToDevice) == hipSuccess) &&
       hipMemcpy(p->d_dtab, dtab.data(), sizeof(grdma_h2_link_deframe) * n, hipMemcpyHostToDevice) == hipSuccess &&
       hipEventCreateWithFlags(&p->framed, hipEventDisableTiming) == hipSuccess &&
       hipEventCreateWithFlags(&p->job_done, hipEventDisableTiming) == hipSuccess &&
       hipEventCreateWithFlags(&p->deframed, hipEventDisableTiming) == hipSuccess &&
       hipEventCreate(&p->t_f0) == hipSuccess && hipEventCreate(&p->t_f1) == hipSuccess &&
       hipEventCreate(&p->t_d0) == hipSuccess && hipEventCreate(&p->t_d1) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    grdma_h2_group_pipe_destroy(p);
    grdma_fail_msg(GRDMA_ERR_HIP, "h2 group pipe: device allocation failed");
    return nullptr;
  }
  const char* fe = getenv("GRDMA_H2_PIPE_FUSED");
  if (!fe || atoi(fe) != 0) {
    grdma_job_hook pre[2], post;
    memset(pre, 0, sizeof(pre));
    memset(&post, 0, sizeof(post));
    uint32_t n_pre = 1;
    if (rspecs) {  // a linear chain in front of the job's first round, as the single reply pipe's
      pre[0].fn = (const void*)k_h2_reply_plan_links;
      pre[0].grid = n;
      pre[0].threads = PLAN_THREADS;
      pre[1].fn = (const void*)k_h2_reply_emit_links;
      pre[1].grid = H2R_GRID;
      pre[1].threads = H2_EMIT_THREADS;
      pre[0].args[0] = pre[1].args[0] = (uint64_t)(uintptr_t)p->d_rtab;
      pre[1].args[1] = n;
      n_pre = 2;
    } else {
      pre[0].fn = (const void*)k_h2_frame_links;
      pre[0].grid = p->frame_grid;
      pre[0].threads = H2_EMIT_THREADS;
      pre[0].args[0] = (uint64_t)(uintptr_t)p->d_ftab;
      pre[0].args[1] = n;
    }
    post.fn = (const void*)k_h2_deframe_links;
    post.grid = n;
    post.threads = H2_DEFRAME_THREADS;
    post.args[0] = (uint64_t)(uintptr_t)p->d_dtab;
    if (grdma_job_set_hooks(job, pre, n_pre, &post, 1) != 0) {
      grdma_h2_group_pipe_destroy(p);
      return nullptr;
    }
    memcpy(p->pre, pre, sizeof(pre));
    p->n_pre = n_pre;
    p->post = post;
    p->fused = true;
  }
  return p;
}

grdma_h2_group_pipe* grdma_h2_group_pipe_create(grdma_stream_job* job, const grdma_h2_link_spec* specs, uint32_t n,
                                                uint32_t max_frame) {
  if (!specs) return h2_group_refuse(nullptr, "h2 group pipe: a job and 1 .. GRDMA_H2_BATCH_MAX link specs");
  return h2_group_create(job, specs, nullptr, n, max_frame);
}

grdma_h2_group_pipe* grdma_h2_group_pipe_create_reply(grdma_stream_job* job_back, const grdma_h2_reply_link_spec* specs,
                                                      uint32_t n) {
  if (!specs) return h2_group_refuse(nullptr, "h2 group pipe: a job and 1 .. GRDMA_H2_BATCH_MAX link specs");
  return h2_group_create(job_back, nullptr, specs, n, 0);
}

// a group reply pipe lets go of its replies (its streams are synchronised: nothing gathers from the sources' arenas)
static void h2_group_unbind_replies(grdma_h2_group_pipe* p) {
  for (grdma_h2_reply* r : p->replies) {
    if (r->src->last_read == p->deframed || r->src->last_read == p->job_done) r->src->last_read = nullptr;
    r->src->reply_pipes--;
    r->gpipe = nullptr;
  }
  p->replies.clear();
}

void grdma_h2_group_pipe_destroy(grdma_h2_group_pipe* p) {
  if (!p) return;
  for (const grdma_h2_asm* a : p->asms)
    if (h2_asm_read_by_reply_pipes(a)) return;  // (a reply pipe's job gathers from this pipe's arenas: destroy that one first)
  if (p->launched) {
    hipStreamSynchronize(p->frame_stream);
    hipStreamSynchronize(p->job_stream);
  }
  for (h2_group_link& l : p->links) {
    if (l.parser && l.parser->last_deframed == p->deframed) l.parser->last_deframed = nullptr;  // (synchronised above)
    hipFree(l.d_msgs);
    hipFree(l.d_hdr);
    hipFree(l.d_ev);
  }
  if (p->fused && p->job) grdma_job_set_hooks(p->job, nullptr, 0, nullptr, 0);
  h2_group_unbind_replies(p);
  h2_group_detach(p);
  hipFree(p->d_rtab);
  hipFree(p->d_atab);
  hipFree(p->d_calls);
  hipFree(p->d_ftab);
  hipFree(p->d_dtab);
  hipFree(p->d_fres);
  hipFree(p->d_dres);
  for (hipEvent_t e : {p->framed, p->job_done, p->deframed, p->t_f0, p->t_f1, p->t_d0, p->t_d1})
    if (e) hipEventDestroy(e);
  delete p;
}

int grdma_h2_group_pipe_enqueue(grdma_h2_group_pipe* p) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p) return -GRDMA_ERR_INVALID;
  const uint32_t n = (uint32_t)p->links.size();
  // every parser's state is handed over from its previous deframing (a pipe step or a call on another stream)
  auto wait_parsers = [&]() {
    for (h2_group_link& l : p->links)
      if (l.parser->last_deframed && l.parser->last_stream != p->job_stream &&
          hipStreamWaitEvent(p->job_stream, l.parser->last_deframed, 0) != hipSuccess)
        return false;
    return true;
  };
  auto done = [&]() {
    for (h2_group_link& l : p->links) {
      l.parser->last_stream = p->job_stream;
      l.parser->last_deframed = p->deframed;
    }
    p->launched = true;
  };
  // a reply step reads what the forward steps assembled: behind every distinct source parser's last deframing
  auto wait_sources = [&](hipStream_t st) {
    for (size_t i = 0; i < p->replies.size(); i++) {
      const grdma_h2_parser* fp = p->replies[i]->src->parser;
      bool seen = false;
      for (size_t k = 0; k < i && !seen; k++) seen = p->replies[k]->src->parser == fp;
      if (!seen && fp->last_deframed && fp->last_stream != st && hipStreamWaitEvent(st, fp->last_deframed, 0) != hipSuccess)
        return false;
    }
    return true;
  };
  // ... and a step's release (at the start of its assembly) waits for the last reply step that gathers from the arena
  auto wait_readers = [&]() {
    for (const grdma_h2_asm* a : p->asms)
      if (hipEvent_t rd = h2_asm_last_read(a))
        if (hipStreamWaitEvent(p->job_stream, rd, 0) != hipSuccess) return false;
    return true;
  };
  auto sources_read_until = [&](hipEvent_t read_done) {
    for (grdma_h2_reply* r : p->replies) r->src->last_read = read_done;
  };
  if (p->fused) {  // one graph launch: the framing kernel(s) -> the job's rounds -> k_h2_deframe_links [-> the six k_h2_asm_*_links]
    if (!wait_parsers() || !wait_sources(p->job_stream) || !wait_readers()) return -GRDMA_ERR_HIP;
    const int rc = grdma_stream_job_launch(p->job);
    if (rc < 0) return rc;
    if (hipEventRecord(p->deframed, p->job_stream) != hipSuccess) return -GRDMA_ERR_HIP;
    sources_read_until(p->deframed);
    p->timed = false;
    done();
    return 0;
  }
  p->timed = true;
  // framing overwrites the slice tables the job's previous step read
  if (p->launched && hipStreamWaitEvent(p->frame_stream, p->job_done, 0) != hipSuccess) return -GRDMA_ERR_HIP;
  if (hipMemsetAsync(p->d_fres, 0, sizeof(grdma_h2_frame_result) * n, p->frame_stream) != hipSuccess) return -GRDMA_ERR_HIP;
  if (!wait_sources(p->frame_stream)) return -GRDMA_ERR_HIP;
  hipEventRecord(p->t_f0, p->frame_stream);
  if (p->d_rtab) {
    hipLaunchKernelGGL(k_h2_reply_plan_links, dim3(n), dim3(PLAN_THREADS), 0, p->frame_stream, (const h2r_link*)p->d_rtab);
    hipLaunchKernelGGL(k_h2_reply_emit_links, dim3(H2R_GRID), dim3(H2_EMIT_THREADS), 0, p->frame_stream,
                       (const h2r_link*)p->d_rtab, n);
  } else {
    hipLaunchKernelGGL(k_h2_frame_links, dim3(p->frame_grid), dim3(H2_EMIT_THREADS), 0, p->frame_stream,
                       (const grdma_h2_link_frame*)p->d_ftab, n);
  }
  hipEventRecord(p->t_f1, p->frame_stream);
  if (hipEventRecord(p->framed, p->frame_stream) != hipSuccess) return -GRDMA_ERR_HIP;
  if (hipStreamWaitEvent(p->job_stream, p->framed, 0) != hipSuccess) return -GRDMA_ERR_HIP;
  if (!wait_readers()) return -GRDMA_ERR_HIP;
  const int rc = grdma_stream_job_launch(p->job);
  if (rc < 0) return rc;
  if (hipEventRecord(p->job_done, p->job_stream) != hipSuccess) return -GRDMA_ERR_HIP;
  sources_read_until(p->job_done);
  // the deframing goes behind the job on the job's stream (csrc: why the single pipe does the same by default)
  if (!wait_parsers()) return -GRDMA_ERR_HIP;
  hipEventRecord(p->t_d0, p->job_stream);
  hipLaunchKernelGGL(k_h2_deframe_links, dim3(n), dim3(H2_DEFRAME_THREADS), 0, p->job_stream,
                     (const grdma_h2_link_deframe*)p->d_dtab);
  if (p->n_asm) h2_asm_links_enqueue(p->d_atab, p->n_asm, p->job_stream);
  hipEventRecord(p->t_d1, p->job_stream);
  if (hipEventRecord(p->deframed, p->job_stream) != hipSuccess) return -GRDMA_ERR_HIP;
  done();
  return 0;
}

static int h2_group_wait(grdma_h2_group_pipe* p) {
  if (hipStreamSynchronize(p->frame_stream) != hipSuccess || hipStreamSynchronize(p->job_stream) != hipSuccess) return -GRDMA_ERR_HIP;
  return 0;
}

int grdma_h2_group_pipe_sync(grdma_h2_group_pipe* p, uint64_t* out, uint64_t out_words) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !out || out_words < 14 * p->links.size()) return -GRDMA_ERR_INVALID;
  if (int rc = h2_group_wait(p)) return rc;
  const size_t n = p->links.size();
  std::vector<grdma_h2_frame_result> fr(n);
  std::vector<grdma_h2_deframe_result> dr(n);
  if (hipMemcpy(fr.data(), p->d_fres, sizeof(grdma_h2_frame_result) * n, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(dr.data(), p->d_dres, sizeof(grdma_h2_deframe_result) * n, hipMemcpyDeviceToHost) != hipSuccess)
    return -GRDMA_ERR_HIP;
  for (size_t i = 0; i < p->replies.size(); i++)  // (a link's overflow 2: its step had another shape than the recorded one)
    if (!h2_reply_result(p->replies[i], &fr[i])) return -GRDMA_ERR_HIP;
  float fms = 0, dms = 0;
  uint64_t f_us = 0, d_us = 0;
  if (p->launched && p->timed && hipEventElapsedTime(&fms, p->t_f0, p->t_f1) == hipSuccess) f_us = (uint64_t)(fms * 1e3f);
  if (p->launched && p->timed && hipEventElapsedTime(&dms, p->t_d0, p->t_d1) == hipSuccess) d_us = (uint64_t)(dms * 1e3f);
  for (size_t i = 0; i < n; i++) {
    uint64_t* o = out + 14 * i;
    o[0] = fr[i].nslices;
    o[1] = fr[i].overflow;
    o[2] = dr[i].nevents;
    o[3] = dr[i].overflow;
    o[4] = dr[i].slices_done;
    o[5] = (uint64_t)dr[i].error;
    o[6] = f_us;  // (the batch's, repeated)
    o[7] = d_us;
    o[8] = dr[i].bulk_steps;
    o[9] = dr[i].bulk_frames;
    o[10] = dr[i].t_wait;
    o[11] = dr[i].t_bulk;
    o[12] = dr[i].t_total;
    o[13] = dr[i].t_serial;
  }
  return 0;
}

int64_t grdma_h2_group_pipe_events(grdma_h2_group_pipe* p, uint32_t i, grdma_h2_event* out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || i >= p->links.size() || (!out && cap)) return -GRDMA_ERR_INVALID;
  if (int rc = h2_group_wait(p)) return rc;
  grdma_h2_deframe_result dr;
  if (hipMemcpy(&dr, p->d_dres + i, sizeof(dr), hipMemcpyDeviceToHost) != hipSuccess) return -GRDMA_ERR_HIP;
  const uint64_t m = std::min<uint64_t>(dr.nevents, p->links[i].ev_cap);
  if (m > cap) return -GRDMA_ERR_CAPACITY;
  if (m && hipMemcpy(out, p->links[i].d_ev, sizeof(grdma_h2_event) * m, hipMemcpyDeviceToHost) != hipSuccess) return -GRDMA_ERR_HIP;
  return (int64_t)m;
}

int64_t grdma_h2_group_pipe_slice_table(grdma_h2_group_pipe* p, uint32_t i, grdma_slice* out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || i >= p->links.size() || (!out && cap)) return -GRDMA_ERR_INVALID;
  const h2_group_link& l = p->links[i];
  if (l.count > cap) return -GRDMA_ERR_CAPACITY;
  if (int rc = h2_group_wait(p)) return rc;
  if (l.count && hipMemcpy(out, l.d_sges, sizeof(grdma_sge) * l.count, hipMemcpyDeviceToHost) != hipSuccess) return -GRDMA_ERR_HIP;
  return (int64_t)l.count;
}

// ---- the message assembler on many links (k_h2_asm_*_links, csrc/grdma_h2_asm.h) -----------------------------------
// Six launches for any number of links: the plan's one-workgroup stages of the links run side by side.
static_assert(H2A_LINKS_MAX == GRDMA_H2_BATCH_MAX, "the assembler's link table is the batch's");

static void h2_asm_links_enqueue(const h2a_link* d_tab, uint32_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_h2_asm_tiles_links, dim3(n * H2A_LINK_GRID), dim3(H2A_THREADS), 0, st, d_tab, n);
  hipLaunchKernelGGL(k_h2_asm_carry_links, dim3(n), dim3(H2A_ONE_THREADS), 0, st, d_tab);
  hipLaunchKernelGGL(k_h2_asm_begin_links, dim3(n * H2A_LINK_GRID), dim3(H2A_THREADS), 0, st, d_tab, n);
  hipLaunchKernelGGL(k_h2_asm_bytes_links, dim3(n * H2A_LINK_GRID), dim3(H2A_THREADS), 0, st, d_tab, n);
  hipLaunchKernelGGL(k_h2_asm_finish_links, dim3(n), dim3(H2A_ONE_THREADS), 0, st, d_tab);
  hipLaunchKernelGGL(k_h2_asm_copy_links, dim3(H2A_GRID), dim3(H2A_THREADS), 0, st, d_tab, n);
}

// the same six kernels as post hooks of a fused group pipe's graph, behind k_h2_deframe_links
static uint32_t h2_asm_links_hooks(const h2a_link* d_tab, uint32_t n, grdma_job_hook* out) {
  const void* fns[6] = {(const void*)k_h2_asm_tiles_links, (const void*)k_h2_asm_carry_links, (const void*)k_h2_asm_begin_links,
                        (const void*)k_h2_asm_bytes_links, (const void*)k_h2_asm_finish_links, (const void*)k_h2_asm_copy_links};
  const uint32_t grids[6] = {n * H2A_LINK_GRID, n, n * H2A_LINK_GRID, n * H2A_LINK_GRID, n, H2A_GRID};
  const uint32_t threads[6] = {H2A_THREADS, H2A_ONE_THREADS, H2A_THREADS, H2A_THREADS, H2A_ONE_THREADS, H2A_THREADS};
  for (int k = 0; k < 6; k++) {
    memset(&out[k], 0, sizeof(out[k]));
    out[k].fn = fns[k];
    out[k].grid = grids[k];
    out[k].threads = threads[k];
    out[k].args[0] = (uint64_t)(uintptr_t)d_tab;
    out[k].args[1] = n;
  }
  return 6;
}

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
  for (uint32_t i = 0; i < n_items; i++) {
    grdma_h2_parser* p = items[i].parser;
    if (p->last_deframed && p->last_stream != st && hipStreamWaitEvent(st, p->last_deframed, 0) != hipSuccess) return -GRDMA_ERR_HIP;
  }
  if (hipMemcpyAsync(d, up.data(), o_ev, hipMemcpyHostToDevice, st) != hipSuccess) return -GRDMA_ERR_HIP;
  hipEventRecord(hc->e0, st);
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_h2_deframe_links, dim3(n_items), dim3(H2_DEFRAME_THREADS), 0, st, (const grdma_h2_link_deframe*)d);
  hipEventRecord(hc->e1, st);
  // the assembly: the plan (five kernels), then the copy, timed apart
  const h2a_link* d_atab = reinterpret_cast<const h2a_link*>(d + o_atab);
  hipEventRecord(lc->e0, st);
  hipLaunchKernelGGL(k_h2_asm_tiles_links, dim3(n_items * H2A_LINK_GRID), dim3(H2A_THREADS), 0, st, d_atab, n_items);
  hipLaunchKernelGGL(k_h2_asm_carry_links, dim3(n_items), dim3(H2A_ONE_THREADS), 0, st, d_atab);
  hipLaunchKernelGGL(k_h2_asm_begin_links, dim3(n_items * H2A_LINK_GRID), dim3(H2A_THREADS), 0, st, d_atab, n_items);
  hipLaunchKernelGGL(k_h2_asm_bytes_links, dim3(n_items * H2A_LINK_GRID), dim3(H2A_THREADS), 0, st, d_atab, n_items);
  hipLaunchKernelGGL(k_h2_asm_finish_links, dim3(n_items), dim3(H2A_ONE_THREADS), 0, st, d_atab);
  hipEventRecord(lc->e1, st);
  hipLaunchKernelGGL(k_h2_asm_copy_links, dim3(H2A_GRID), dim3(H2A_THREADS), 0, st, d_atab, n_items);
  hipEventRecord(lc->e2, st);
  if (hipGetLastError() != hipSuccess) {
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
    const h2a_dev& h = hs[i];
    const uint64_t m = res[i].nevents < it.cap ? res[i].nevents : it.cap;
    if (it.events_out && m) memcpy(it.events_out, ev + a_ev, sizeof(grdma_h2_event) * m);
    it.h2_error = (int)res[i].error;
    it.n_events = res[i].overflow ? -(int64_t)GRDMA_ERR_CAPACITY : (int64_t)m;
    it.assembler->plan_ms = plan_ms;  // (the batch's, repeated)
    it.assembler->copy_ms = copy_ms;
    if (res[i].overflow || h.skip || h.ndesc > it.msgs_cap || h.ndesc > h.desc_cap) {
      it.n_msgs = -(int64_t)GRDMA_ERR_CAPACITY;
    } else {
      it.n_msgs = (int64_t)h.ndesc;
      if (h.ndesc) {
        if (hipMemcpyAsync(it.msgs_out, h.desc, sizeof(grdma_h2_rx_msg) * h.ndesc, hipMemcpyDeviceToHost, st) != hipSuccess)
          return -GRDMA_ERR_HIP;
        more = true;
      }
    }
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
  for (uint32_t i = 0; i < n; i++) {
    grdma_h2_parser* p = asms[i]->parser;
    if (p->last_deframed && hipStreamWaitEvent(st, p->last_deframed, 0) != hipSuccess) return -GRDMA_ERR_HIP;
  }
  if (lc->rel_pending && hipEventSynchronize(lc->rel_up) != hipSuccess) return -GRDMA_ERR_HIP;
  for (uint32_t i = 0; i < n; i++) lc->h_rel[i] = h2a_link_release{asms[i]->d, counts[i]};
  if (hipMemcpyAsync(lc->d_rel, lc->h_rel, sizeof(h2a_link_release) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipEventRecord(lc->rel_up, st) != hipSuccess)
    return -GRDMA_ERR_HIP;
  lc->rel_pending = true;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_h2_asm_release_links, dim3(n), dim3(64), 0, st, (const h2a_link_release*)lc->d_rel);
  return hipGetLastError() == hipSuccess ? 0 : -GRDMA_ERR_HIP;
}

static void h2_group_detach(grdma_h2_group_pipe* p) {
  for (grdma_h2_asm*& a : p->asms)
    if (a) {
      a->parser->asm_attached--;
      a->attached--;
      a = nullptr;
    }
  p->n_asm = 0;
}

int grdma_h2_group_pipe_attach_assemblers(grdma_h2_group_pipe* p, grdma_h2_asm* const* asms, uint32_t n) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !asms) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: a pipe and an assembler list");
  if (n != p->links.size()) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: one assembler entry per link spec");
  if (p->n_asm) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: assemblers are attached already");
  uint32_t have = 0;
  for (uint32_t i = 0; i < n; i++) {
    grdma_h2_asm* a = asms[i];
    if (!a) continue;
    if (a->parser != p->links[i].parser) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: an assembler of another parser than its link's");
    if (a->attached || a->parser->asm_attached) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: an assembler attached already");
    for (uint32_t k = 0; k < i; k++)
      if (asms[k] == a) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: the same assembler twice");
    have++;
  }
  if (!have) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: no assembler in the list");
  if (p->launched && h2_group_wait(p) != 0) return -GRDMA_ERR_HIP;
  std::vector<h2a_call> calls;
  std::vector<h2a_link> tab;
  if ((!p->d_atab && hipMalloc((void**)&p->d_atab, sizeof(h2a_link) * n) != hipSuccess) ||
      (!p->d_calls && hipMalloc((void**)&p->d_calls, sizeof(h2a_call) * n) != hipSuccess))
    return -GRDMA_ERR_HIP;
  for (uint32_t i = 0; i < n; i++) {
    if (!asms[i]) continue;
    const h2_group_link& l = p->links[i];
    if (!h2_asm_prepare(asms[i], l.ev_cap ? l.ev_cap : 1)) return -GRDMA_ERR_HIP;
    // (a step first releases everything reported before it, as a single pipe's does)
    tab.push_back(h2a_link{asms[i]->d, p->d_calls + calls.size()});
    calls.push_back(h2a_call{l.d_ev, p->d_dres + i, l.d_slices, l.dst, l.ev_cap, 1});
  }
  if (hipMemcpy(p->d_calls, calls.data(), sizeof(h2a_call) * have, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(p->d_atab, tab.data(), sizeof(h2a_link) * have, hipMemcpyHostToDevice) != hipSuccess)
    return -GRDMA_ERR_HIP;
  if (p->fused) {
    grdma_job_hook post[7];
    post[0] = p->post;
    const uint32_t n_post = 1 + h2_asm_links_hooks(p->d_atab, have, post + 1);
    if (grdma_job_set_hooks(p->job, p->pre, p->n_pre, post, n_post) != 0) return -GRDMA_ERR_HIP;
  }
  p->asms.assign(asms, asms + n);
  p->n_asm = have;
  for (grdma_h2_asm* a : p->asms)
    if (a) {
      a->attached++;
      a->parser->asm_attached++;
    }
  return 0;
}

int64_t grdma_h2_group_pipe_messages(grdma_h2_group_pipe* p, uint32_t i, grdma_h2_rx_msg* out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || i >= p->asms.size() || !p->asms[i] || (!out && cap)) return -GRDMA_ERR_INVALID;
  if (int rc = h2_group_wait(p)) return rc;
  h2a_dev h;
  if (hipMemcpy(&h, p->asms[i]->d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -GRDMA_ERR_HIP;
  if (h.skip || h.ndesc > cap || h.ndesc > h.desc_cap) return -GRDMA_ERR_CAPACITY;
  if (h.ndesc && hipMemcpy(out, h.desc, sizeof(grdma_h2_rx_msg) * h.ndesc, hipMemcpyDeviceToHost) != hipSuccess)
    return -GRDMA_ERR_HIP;
  return (int64_t)h.ndesc;
}

}  // extern "C"
