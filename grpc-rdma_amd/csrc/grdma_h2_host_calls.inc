// HTTP/2 on the device: the standalone and the batch calls.  Included by csrc/grdma_h2.hip (inside its extern "C" block),
// behind the stage builders and in front of the pipes (csrc/grdma_h2_host_pipe.inc), which build on the parser, the
// assembler, the reply and the ledger as they are defined here.
//
// Every call runs on the one stream of the process (h2_ctx), one at a time, and has one shape: uploads, launches with
// stamps around the timed ones, downloads, ONE synchronise, elapsed times.  A call describes itself in an h2_call;
// h2_call_run is the only place that knows the order and what a refused launch leads to.  An entry point keeps what is
// its own: the argument checks, the growth of its scratch, the reading of its result block.

// ---- the call runner -----------------------------------------------------------------------------------------------------
struct h2_xfer { void* dst; const void* src; size_t bytes; };  // one copy; bytes 0: none.  An upload without src clears dst.
struct h2_span { const grdma_job_hook* recs; size_t n; };      // records of a stage, launched in order
static h2_span h2_all(const h2_stage& s) { return {s.data(), s.size()}; }
// an assembler's stage in two: the plan, and the copy behind it (the standalone calls time them apart)
static h2_span h2_asm_plan(const h2_stage& s) { return {s.data(), H2_ASM_PLAN}; }
static h2_span h2_asm_copy(const h2_stage& s) { return {s.data() + H2_ASM_PLAN, s.size() - H2_ASM_PLAN}; }
struct h2_call {
  const char* refused;         // grdma_last_error when the runtime refuses a launch
  std::vector<h2_xfer> up;     // host to device, in front of the launches
  h2_span lead;                // launched in front of the first stamp: not timed
  std::vector<h2_span> timed;  // at most 3 sections, a stamp in front of each and one behind the last
  std::vector<h2_xfer> down;   // device to host, behind the launches
  float ms[3];                 // out: what each timed section took (0 where the runtime cannot tell)
};

// The runtime refused a launch on st: what the call enqueued ends before the caller's buffers go; the call fails with a message.
static int h2_refused(hipStream_t st, const char* what) {
  hipStreamSynchronize(st);
  return grdma_fail_msg(GRDMA_ERR_HIP, what);
}

// 0, or -GRDMA_ERR_HIP: with c->refused as message for a refused launch, without one for a failed copy or synchronise
static int h2_call_run(h2_host_ctx* hc, h2_call* c) {
  hipStream_t st = hc->stream;
  for (const h2_xfer& x : c->up)
    if (x.bytes && (x.src ? hipMemcpyAsync(x.dst, x.src, x.bytes, hipMemcpyHostToDevice, st) : hipMemsetAsync(x.dst, 0, x.bytes, st)) != hipSuccess)
      return -GRDMA_ERR_HIP;
  const size_t k = c->timed.size();
  hipError_t launched = h2_launch(c->lead.recs, c->lead.n, st);
  for (size_t i = 0; i < k && launched == hipSuccess; i++) {
    hipEventRecord(hc->stamp[i], st);
    launched = h2_launch(c->timed[i].recs, c->timed[i].n, st);
  }
  if (launched != hipSuccess) return h2_refused(st, c->refused);
  if (k) hipEventRecord(hc->stamp[k], st);
  for (const h2_xfer& x : c->down)
    if (x.bytes && hipMemcpyAsync(x.dst, x.src, x.bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return -GRDMA_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess) return -GRDMA_ERR_HIP;
  for (size_t i = 0; i < k; i++)
    if (hipEventElapsedTime(&c->ms[i], hc->stamp[i], hc->stamp[i + 1]) != hipSuccess) c->ms[i] = 0;
  return 0;
}

// device memory read to the host on the stream of the calls, behind whatever they enqueued, and synchronised
static bool h2_read(void* dst, const void* dev_src, size_t bytes) {
  h2_host_ctx* hc = h2_ctx();
  return hc && hipMemcpyAsync(dst, dev_src, bytes, hipMemcpyDeviceToHost, hc->stream) == hipSuccess &&
         hipStreamSynchronize(hc->stream) == hipSuccess;
}

// The words [off_begin, off_end) of a host mirror go to the device block they mirror, on st or with a blocking copy when
// st is NULL: the configuration words of an assembler, a reply or a ledger (the rest of the block is the device's).
static bool h2_push_words(void* dev, const void* host, size_t off_begin, size_t off_end, hipStream_t st) {
  uint8_t* dst = static_cast<uint8_t*>(dev) + off_begin;
  const uint8_t* src = static_cast<const uint8_t*>(host) + off_begin;
  const size_t len = off_end - off_begin;
  return (st ? hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, st) : hipMemcpy(dst, src, len, hipMemcpyHostToDevice)) == hipSuccess;
}
// ... as an upload of a call
static h2_xfer h2_words(void* dev, const void* host, size_t off_begin, size_t off_end) {
  return {static_cast<uint8_t*>(dev) + off_begin, static_cast<const uint8_t*>(host) + off_begin, off_end - off_begin};
}
// the n result words at off of a device block, as a download of a call
static h2_xfer h2_result(uint64_t* dst, const void* dev, size_t off, size_t n = 8) {
  return {dst, static_cast<const uint8_t*>(dev) + off, n * sizeof(uint64_t)};
}

// ---- what a facility's single call and its batch share ---------------------------------------------------------------------
// The rules of a facility stand once, in static functions over ONE item: a refusal (a reason without the facility's
// name, NULL when there is none), the call block or words, the target words, and what the host keeps behind a call that
// ran.  The single entry point is those steps around its own stage; the batch is the same steps in a loop around the
// links stage, inside an h2_batch (below).
static int h2_invalid(const char* who, const char* why) {
  char msg[256];
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  return grdma_fail_msg(GRDMA_ERR_INVALID, msg);  // (copies it)
}
// a refused creation
static std::nullptr_t h2_no(const char* why) {
  grdma_fail_msg(GRDMA_ERR_INVALID, why);
  return nullptr;
}

// where a call writes frames: a slice table and a header arena in device memory
static const char* h2_bad_target(const void* d_slices_out, uint64_t slices_cap, const void* d_hdr_arena, uint64_t hdr_cap) {
  if (!d_slices_out || !slices_cap || !d_hdr_arena || !hdr_cap || ((uintptr_t)d_slices_out & 15) || ((uintptr_t)d_hdr_arena & 15))
    return "a null, zero or misaligned slice table or header arena";
  return nullptr;
}

// A follower of a parser's standalone deframings: the ledger, the send windows and the control-reply writer each read
// what the last grdma_h2_deframe / grdma_h2_deframe_messages left in the parser's buffers, every call once.
struct h2_follow {
  grdma_h2_parser* parser = nullptr;  // NULL once the parser is gone: the follower's device block points into the parser's
  uint64_t taken = 0;                 // parser->standalone_calls of the last call taken
  float last_ms = 0;                  // of the last call's stage
};
// The parser of f is being destroyed: standalone calls on the stream of the calls have ended, and from now on f refuses
// every call but destroy.  (A ledger attached to a pipe stays with the pipe, whose parser must outlive it.)
static void h2_follow_parser_gone(h2_follow* f) {
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);
  f->parser = nullptr;
}
// positions32: the facility keeps event positions in 32 bits
static const char* h2_follow_refusal(const h2_follow& f, const char* taken_already, bool positions32) {
  const grdma_h2_parser* p = f.parser;
  if (!p) return "the parser is gone";
  if (p->standalone_calls == 0) return "the parser has deframed nothing yet";
  if (f.taken == p->standalone_calls) return taken_already;
  if (positions32 && p->standalone_ev_cap >= 0xfffffff0ull) return "event positions are 32 bits";
  return nullptr;
}
// The parser's last standalone deframing as f's call block names it; each facility's block takes the members it has.
struct h2_deframed {
  const grdma_h2_event* ev;
  const grdma_h2_deframe_result* res;
  const grdma_slice_out* sl;
  const uint8_t* arena;
  uint64_t ev_cap, nsl;
  uint64_t skipped;  // a deframing in front of this one was never taken
  operator h2fc_call() const { return {ev, res, ev_cap}; }
  operator h2sw_call() const { return {ev, res, sl, arena, ev_cap, nsl, skipped}; }
  operator h2ctl_call() const { return {ev, res, sl, arena, ev_cap, nsl, skipped}; }
  operator h2hp_call() const { return {ev, res, sl, arena, ev_cap, nsl, skipped}; }
};
static h2_deframed h2_follow_deframed(const h2_follow& f) {
  const grdma_h2_parser* p = f.parser;
  return {p->d_ev, p->d_res, p->d_sl, p->standalone_arena, p->standalone_ev_cap, p->standalone_nsl,
          p->standalone_calls > f.taken + 1 ? 1ull : 0ull};
}
// behind a call of f that ran
static void h2_follow_ran(h2_follow* f, float ms, bool taken = true) {
  f->last_ms = ms;
  if (taken) f->taken = f->parser->standalone_calls;
}

static double g_h2_last_kernel_us = 0;
static uint64_t g_h2_last_boundary_steps = 0;
static uint64_t g_h2_last_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

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
  const h2_stage framing = h2_stage_frame(d_msgs, n, max_frame, reinterpret_cast<grdma_sge*>(d_slices_out), slices_cap,
                                          static_cast<uint8_t*>(d_hdr_arena), hdr_cap, d_pos, d_res);
  h2_call c{"grdma_h2_frame_messages: a launch was rejected",
            {{d_msgs, tmp.data(), sizeof(grdma_h2_msg_dev) * n}, {d_res, nullptr, sizeof(grdma_h2_frame_result)}}, {}, {h2_all(framing)},
            {{&h_res, d_res, sizeof(h_res)}}};
  if (int rc = h2_call_run(hc, &c)) return rc;
  g_h2_last_kernel_us = 1e3 * c.ms[0];
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

static void h2_followers_parser_gone(grdma_h2_parser* p);
void grdma_h2_parser_destroy(grdma_h2_parser* p) {
  if (!p) return;
  h2_followers_parser_gone(p);  // (the ledger, the send windows and the control-reply writer outlive it as husks)
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
  const grdma_job_hook ops = h2_rec(k_h2_table_ops, 1, 1, p->d, p->d_ops, n);
  h2_call c{"h2 parser: the launch of k_h2_table_ops was rejected",
            {{p->d_ops, h.data(), sizeof(grdma_h2_table_op) * n}}, {&ops, 1}, {},
            {{h.data(), p->d_ops, sizeof(grdma_h2_table_op) * n}}};
  if (int rc = h2_call_run(hc, &c)) return rc;
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
  uint64_t v[2];
  if (!h2_read(v, reinterpret_cast<uint8_t*>(p->d_chunks) + offsetof(grdma_h2_chunks, n_planned), sizeof(v))) return -GRDMA_ERR_HIP;
  out[0] = v[0];
  out[1] = v[1];
  return 0;
}
// profiling aid: the phase stamps of the last chunked call, (H2_KMAX + 1) rows of 8 (csrc/grdma_h2_kernels.h)
int grdma_h2_parser_chunk_dbg(grdma_h2_parser* p, uint64_t* out, uint64_t cap_words) {
  if (!p || !out || !p->d_chunks) return -GRDMA_ERR_INVALID;
  const uint64_t words = std::min<uint64_t>(cap_words, (H2_KMAX + 1) * 8);
  if (!h2_read(out, reinterpret_cast<uint8_t*>(p->d_chunks) + offsetof(grdma_h2_chunks, dbg), words * 8)) return -GRDMA_ERR_HIP;
  return (int)words;
}
int64_t grdma_h2_parser_live_streams(grdma_h2_parser* p) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p) return -GRDMA_ERR_INVALID;
  grdma_h2_parser_dev h;
  if (!h2_read(&h, p->d, sizeof(h))) return -GRDMA_ERR_HIP;
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
  const bool chunked = n >= H2_CHUNK_MIN_SLICES && h2_chunks_prepare(p, cap, hc->stream);
  const h2_stage deframing = h2_stage_deframe(p, static_cast<const uint8_t*>(d_arena), p->d_sl, n, p->d_ev, cap, p->d_res, chunked);
  h2_call c{"grdma_h2_deframe: a launch was rejected",
            {{p->d_sl, slices, sizeof(grdma_slice_out) * n}}, {}, {h2_all(deframing)},
            {{&h_res, p->d_res, sizeof(h_res)}}};
  if (int rc = h2_call_run(hc, &c)) return rc;
  g_h2_last_kernel_us = 1e3 * c.ms[0];
  g_h2_last_boundary_steps = h_res.boundary_steps;
  {
    const uint64_t st[8] = {h_res.bulk_steps, h_res.bulk_frames, h_res.boundary_steps, h_res.t_wait,
                            h_res.t_bulk, h_res.t_boundary, h_res.t_serial, h_res.t_total};
    for (int i = 0; i < 8; i++) g_h2_last_stats[i] = st[i];
  }
  const uint64_t m = h_res.nevents < cap ? h_res.nevents : cap;
  if (m && !h2_read(events_out, p->d_ev, sizeof(grdma_h2_event) * m)) return -GRDMA_ERR_HIP;
  if (h2_error) *h2_error = (int)h_res.error;
  p->standalone_calls++;
  p->standalone_ev_cap = cap;
  p->standalone_arena = static_cast<const uint8_t*>(d_arena);
  p->standalone_nsl = n;
  return h_res.overflow ? -GRDMA_ERR_CAPACITY : (int64_t)m;
}

// ---- the delivered slices of many transports in one launch (k_h2_deframe_links) ---------------------------------
// One device block per process holds a call (its layout: csrc/grdma_h2_block.h): [table | slice lists | zeroed results]
// go up in one copy, [results | event segments] come down in one copy, the kernel in between.  Nothing per item returns
// to the host.  The download moves every item's whole event capacity, not the events produced (their number is only
// known behind it): callers give tight caps.  The block is process-global and unguarded: one call at a time (as the
// other grdma_h2_* calls, which share one stream and its stamps).
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

// The scaffold of a batch call whose block is [table | one block per item] (the ledgers', the send windows', the
// writers', the header decoders', the windowed replies' and the replies'): begin, item for each item, open, the facility's per-item steps
// (which fill the image and add each item's own uploads, downloads and parsers to wait for), run.
struct h2_batch {
  const char* who;   // "h2 ... batch": leads every refusal
  const char* noun;  // what an item names
  const char* launch_refused;  // grdma_last_error when the runtime refuses a launch
  h2_host_ctx* hc = nullptr;
  uint8_t* d = nullptr;      // the block in device memory: the table at d, and behind open() the items' blocks at d + blocks
  uint64_t blocks = 0;
  std::vector<uint8_t> up;   // its host image, zeroed (a result block never reports another call's)
  std::vector<const void*> seen;
  std::vector<const grdma_h2_parser*> behind;  // the call goes behind each one's last deframing by a pipe (another stream)
  h2_call c{};

  int begin(bool arrays, uint32_t n_items) {
    if (!arrays || n_items == 0 || n_items > GRDMA_H2_BATCH_MAX) return h2_invalid(who, "1 .. GRDMA_H2_BATCH_MAX items");
    seen.reserve(n_items);
    behind.reserve(2 * (size_t)n_items);
    return 0;
  }
  // one item per object; why: what the facility's own rules refuse the item for (an item without object among them)
  int item(const void* obj, const char* why) {
    for (const void* s : seen)
      if (obj && s == obj) {
        char twice[96];
        snprintf(twice, sizeof(twice), "the same %s twice", noun);
        return h2_invalid(who, twice);
      }
    seen.push_back(obj);
    return why ? h2_invalid(who, why) : 0;
  }
  // a block of `total` bytes whose first `end` go up (a layout of the caller's own)
  int reserve(uint64_t end, uint64_t total) {
    hc = h2_ctx();
    if (!hc || !h2_batch_reserve(total, hc->stream)) return -GRDMA_ERR_HIP;
    d = g_batch.d;
    up.assign(end, 0);
    c.up.reserve(1 + 3 * seen.size());
    c.down.reserve(1 + 2 * seen.size());
    c.up.push_back({d, up.data(), up.size()});
    return 0;
  }
  int open(uint64_t link_bytes, uint64_t block_bytes, uint32_t n_items) {
    const h2_fc_block L = h2_fc_block_layout(link_bytes, block_bytes, n_items);
    blocks = L.calls;
    return reserve(L.end, L.total);
  }
  // 0, or what h2_call_run returns; c.ms: what the timed sections took
  int run(std::vector<h2_span> timed) {
    for (const grdma_h2_parser* p : behind)
      if (!h2_wait_parser(hc->stream, p)) return -GRDMA_ERR_HIP;
    c.refused = launch_refused;
    c.timed = std::move(timed);
    return h2_call_run(hc, &c);
  }
  // a further run of the same call over the block as it stands on the device (the header decoders' second step): the
  // transfers and the waits of the run before are done with
  void next() {
    c.up.clear();
    c.down.clear();
    behind.clear();
  }
};

static_assert(sizeof(grdma_read_slice) == sizeof(grdma_slice_out) && sizeof(grdma_slice_out) % 16 == 0, "layout");
static h2_deframe_block h2_deframe_batch_layout(uint32_t n_items, uint64_t n_sl, uint64_t n_ev, bool assembled) {
  return h2_deframe_block_layout({sizeof(grdma_h2_link_deframe), sizeof(grdma_slice_out), sizeof(grdma_h2_deframe_result),
                                  sizeof(grdma_h2_event), assembled ? sizeof(h2a_link) : 0, assembled ? sizeof(h2a_call) : 0},
                                 n_items, n_sl, n_ev);
}

// The two deframe batch calls share these: their items begin with the same members.
extern "C++" {
// The front of a block that will lie at d, written to its host image up: the table of k_h2_deframe_links and the items'
// slice lists, packed.  (The results between them and the events stay as up has them: zeroed.)
template <typename Item>
static void h2_batch_pack(const Item* items, uint32_t n_items, const h2_deframe_block& L, uint8_t* up, uint8_t* d) {
  auto* tab = reinterpret_cast<grdma_h2_link_deframe*>(up + L.tab);
  auto* sl = reinterpret_cast<grdma_slice_out*>(up + L.slices);
  uint64_t a_sl = 0, a_ev = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    const Item& it = items[i];
    if (it.n) memcpy(sl + a_sl, it.slices, sizeof(grdma_slice_out) * it.n);
    tab[i].n_step = nullptr;  // (the caller's list: its length is the count)
    tab[i].res = reinterpret_cast<grdma_h2_deframe_result*>(d + L.results) + i;
    tab[i].gp = it.parser->d;
    tab[i].arena = static_cast<const uint8_t*>(it.d_arena);
    tab[i].slices = reinterpret_cast<const grdma_slice_out*>(d + L.slices) + a_sl;
    tab[i].nslices = it.n;
    tab[i].ev = reinterpret_cast<grdma_h2_event*>(d + L.events) + a_ev;
    tab[i].ev_cap = it.cap;
    a_sl += it.n;
    a_ev += it.cap;
  }
}
// Results and events go back to the items from down, the host copy of the block from L.results on (the events only
// where an item has an array for them: the copy need not reach them otherwise).
template <typename Item>
static void h2_batch_hand_back(Item* items, uint32_t n_items, const h2_deframe_block& L, const uint8_t* down) {
  const auto* res = reinterpret_cast<const grdma_h2_deframe_result*>(down);
  const auto* ev = reinterpret_cast<const grdma_h2_event*>(down + (L.events - L.results));
  uint64_t a_ev = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    Item& it = items[i];
    const uint64_t m = res[i].nevents < it.cap ? res[i].nevents : it.cap;
    if (it.events_out && m) memcpy(it.events_out, ev + a_ev, sizeof(grdma_h2_event) * m);
    it.h2_error = (int)res[i].error;
    it.n_events = res[i].overflow ? -(int64_t)GRDMA_ERR_CAPACITY : (int64_t)m;
    a_ev += it.cap;
  }
}
}  // extern "C++"

int grdma_h2_deframe_batch(grdma_h2_deframe_item* items, uint32_t n_items) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 batch", "parser", "h2 batch: a launch was rejected"};
  if (int rc = b.begin(items, n_items)) return rc;
  uint64_t n_sl = 0, n_ev = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_deframe_item& it = items[i];
    const char* why = nullptr;
    if (!it.parser || !it.d_arena || (!it.slices && it.n) || (!it.events_out && it.cap)) why = "an item without parser, arena, slices or event array";
    else if (it.parser->asm_attached) why = "a parser whose assembler is attached to a pipe";
    else if (it.parser->fc) why = "a parser with a flow-control ledger (single transport only)";
    if (int rc = b.item(it.parser, why)) return rc;
    n_sl += it.n;
    n_ev += it.cap;
  }
  const h2_deframe_block L = h2_deframe_batch_layout(n_items, n_sl, n_ev, false);
  if (int rc = b.reserve(L.events, L.total)) return rc;  // ([0, events) goes up)
  std::vector<uint8_t> down(L.total - L.results);
  h2_batch_pack(items, n_items, L, b.up.data(), b.d);
  for (uint32_t i = 0; i < n_items; i++) b.behind.push_back(items[i].parser);
  b.c.down.push_back({down.data(), b.d + L.results, down.size()});
  const h2_stage deframing = h2_stage_deframe_links(reinterpret_cast<const grdma_h2_link_deframe*>(b.d + L.tab), n_items);
  if (int rc = b.run({h2_all(deframing)})) return rc;
  g_h2_last_kernel_us = 1e3 * b.c.ms[0];
  h2_batch_hand_back(items, n_items, L, down.data());
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
  uint64_t calls = 0;              // standalone assembler calls, single and batch (the windowed reply takes each one once)
  float plan_ms = 0, copy_ms = 0;  // of the last standalone call
  uint64_t last_ndesc = 0, last_nev = 0;  // of the last grdma_h2_deframe_messages (grdma_h2_asm_last_call)
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
  return h2_push_words(a->d, &h, offsetof(h2a_dev, scratch_ev), offsetof(h2a_dev, vh), nullptr) && ok;
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
            hipMemcpy(a->d, &h, sizeof(h), hipMemcpyHostToDevice) == hipSuccess;
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
  const bool chunked = n >= H2_CHUNK_MIN_SLICES && h2_chunks_prepare(p, ev_cap, st);
  // the deframing, untimed; then the assembly: the plan and the copy, timed apart
  const h2_stage deframing = h2_stage_deframe(p, static_cast<const uint8_t*>(d_arena), p->d_sl, n, p->d_ev, ev_cap, p->d_res, chunked);
  const h2_stage assembly = h2_stage_asm(a->d, a->d_call);
  grdma_h2_deframe_result h_res;
  h2a_dev h;
  h2_call c{"grdma_h2_deframe_messages: a launch was rejected",
            {{a->d_call, &call, sizeof(call)}, {p->d_sl, slices, sizeof(grdma_slice_out) * n}},
            h2_all(deframing), {h2_asm_plan(assembly), h2_asm_copy(assembly)},
            {{&h_res, p->d_res, sizeof(h_res)}, {&h, a->d, sizeof(h)}}};
  if (int rc = h2_call_run(hc, &c)) return rc;
  a->plan_ms = c.ms[0];
  a->copy_ms = c.ms[1];
  a->calls++;
  p->standalone_calls++;
  p->standalone_ev_cap = ev_cap;
  p->standalone_arena = static_cast<const uint8_t*>(d_arena);
  p->standalone_nsl = n;
  if (h2_error) *h2_error = (int)h_res.error;
  const uint64_t m = h_res.nevents < ev_cap ? h_res.nevents : ev_cap;
  a->last_nev = h_res.overflow ? 0 : m;
  a->last_ndesc = (h_res.overflow || h.skip || h.ndesc > h.desc_cap) ? 0 : h.ndesc;
  if (events_out && m && !h2_read(events_out, p->d_ev, sizeof(grdma_h2_event) * m)) return -GRDMA_ERR_HIP;
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
  return h2_launch(&release, 1, hc->stream) == hipSuccess ? 0 : h2_refused(hc->stream, "grdma_h2_asm_release: the launch was rejected");
}

int grdma_h2_asm_last_call(grdma_h2_asm* a, uint64_t out[4]) {
  if (!a || !out) return -GRDMA_ERR_INVALID;
  if (a->attached) return h2_invalid("h2 assembler", "last_call on an assembler attached to a pipe");
  out[0] = (uint64_t)(uintptr_t)a->h.desc;
  out[1] = a->last_ndesc;
  out[2] = (uint64_t)(uintptr_t)a->parser->d_ev;
  out[3] = a->last_nev;
  return 0;
}

int grdma_h2_asm_stats(grdma_h2_asm* a, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!a || !out) return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  h2a_dev h;
  if (!h2_wait_parser(hc->stream, a->parser) || !h2_read(&h, a->d, sizeof(h))) return -GRDMA_ERR_HIP;
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
  // replies under the peer's windows (csrc/grdma_h2_wr.h): the queue, once grdma_h2_reply_attach_windows has bound it
  h2wr_dev* d_wr = nullptr;
  h2wr_dev wr;                      // host copy of its configuration and call words
  struct grdma_h2_sw* sw = nullptr; // the send windows the replies go out under; NULL once they are gone
  uint64_t taken = 0;               // src->calls of the last source call taken (at the attachment: of the calls before it)
  uint64_t attached_at = 0;         // src->calls at the attachment
  uint64_t pending = 0;             // entries the last call left in the queue
};
static void h2_wr_free(grdma_h2_reply* r);

// where a call frames to, and (a pipe) the shape it must have: the words of an h2r_dev from `out` to the result block
static void h2_reply_target(h2r_dev* h, grdma_sge* out, uint64_t cap, uint8_t* hdr, uint64_t hdr_cap, uint64_t check_shape,
                            uint64_t want_slices, uint64_t want_wire) {
  h->out = out;
  h->cap = cap;
  h->hdr = hdr;
  h->hdr_cap = hdr_cap;
  h->check_shape = check_shape;
  h->want_slices = want_slices;
  h->want_wire = want_wire;
}
// ... in r's host copy, and uploaded (a pipe's)
static bool h2_reply_set_target(grdma_h2_reply* r, grdma_sge* out, uint64_t cap, uint8_t* hdr, uint64_t hdr_cap,
                                uint64_t check_shape, uint64_t want_slices, uint64_t want_wire, hipStream_t st) {
  h2_reply_target(&r->h, out, cap, hdr, hdr_cap, check_shape, want_slices, want_wire);
  return h2_push_words(r->d, &r->h, offsetof(h2r_dev, out), offsetof(h2r_dev, res), st);
}

// (a pipe's reader, behind the pipe's own wait: a blocking copy, not a copy and a synchronise on the stream of the calls --
// the group reply pipe reads once per link and step, and h2_read costs it 3.5 us more each: profiles/h2_host_calls_refactor.md)
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
  memset(&r->wr, 0, sizeof(r->wr));
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
  ok = ok && hipMemcpy(r->d, &h, sizeof(h), hipMemcpyHostToDevice) == hipSuccess;
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
  h2_wr_free(r);
  hipFree(r->h.msgs);
  hipFree(r->h.pos);
  hipFree(r->d_routes);
  hipFree(r->d);
  delete r;
}

// what a call on r into these targets is refused for
static const char* h2_reply_refusal(const grdma_h2_reply* r, const void* d_slices_out, uint64_t slices_cap, const void* d_hdr_arena,
                                    uint64_t hdr_cap) {
  if (!r) return "no reply";
  if (const char* why = h2_bad_target(d_slices_out, slices_cap, d_hdr_arena, hdr_cap)) return why;
  if (r->seq) return "the reply is bound to a reply pipe";
  if (r->d_wr) return "the reply frames under send windows (grdma_h2_reply_frame_windowed)";  // (one message could go out twice)
  if (r->src->attached) return "the source assembler is attached to a pipe or group pipe";
  return nullptr;
}
// a call's result words res and what its stage took, to the caller -> the slice count, -GRDMA_ERR_CAPACITY after an overflow
static int64_t h2_reply_ran(const uint64_t res[8], float ms, uint64_t out[8]) {
  for (int i = 0; i < 7; i++) out[i] = res[i];
  out[7] = (uint64_t)(ms * 1e3f);
  return res[H2R_OVERFLOW] ? -(int64_t)GRDMA_ERR_CAPACITY : (int64_t)res[H2R_SLICES];
}

int64_t grdma_h2_reply_frame(grdma_h2_reply* r, grdma_slice* d_slices_out, uint64_t slices_cap, void* d_hdr_arena,
                             uint64_t hdr_cap, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!out) return h2_invalid("grdma_h2_reply_frame", "no result array");
  if (const char* why = h2_reply_refusal(r, d_slices_out, slices_cap, d_hdr_arena, hdr_cap)) return h2_invalid("grdma_h2_reply_frame", why);
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  // the stream of grdma_h2_deframe_messages: the call is ordered behind the one it reads
  h2_reply_target(&r->h, reinterpret_cast<grdma_sge*>(d_slices_out), slices_cap, static_cast<uint8_t*>(d_hdr_arena), hdr_cap, 0, 0, 0);
  const h2_stage framing = h2_stage_reply(r->d);
  uint64_t res[8];
  h2_call c{"grdma_h2_reply_frame: a launch was rejected", {h2_words(r->d, &r->h, offsetof(h2r_dev, out), offsetof(h2r_dev, res))}, {},
            {h2_all(framing)}, {h2_result(res, r->d, offsetof(h2r_dev, res))}};
  if (int rc = h2_call_run(hc, &c)) return rc;
  return h2_reply_ran(res, c.ms[0], out);
}

// ---- the replies of many transports in two launches (h2_stage_reply_links) ------------------------------------------
// The batch block of the process holds the call: [table | one h2r_dev per item] goes up in one copy -- the item's
// framer with the item's targets and a zeroed result block; scratch, routes and source stay the reply's own -- and the
// h2r_dev blocks come down in one copy.  One call at a time, as the other batch calls.
int grdma_h2_reply_frame_batch(grdma_h2_reply_item* items, uint32_t n_items) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 reply batch", "reply", "h2 reply batch: a launch was rejected"};
  if (int rc = b.begin(items, n_items)) return rc;
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_reply_item& it = items[i];
    if (int rc = b.item(it.reply, h2_reply_refusal(it.reply, it.d_slices_out, it.slices_cap, it.d_hdr_arena, it.hdr_cap))) return rc;
    // (each reply has scratch of its own, so two of one source could run side by side; the rule is one item per
    // transport, as in the other batch calls)
    for (uint32_t k = 0; k < i; k++)
      if (items[k].reply->src == it.reply->src) return h2_invalid(b.who, "two replies of one source assembler");
  }
  const h2_reply_block L = h2_reply_block_layout(sizeof(h2r_link), sizeof(h2r_dev), n_items);
  if (int rc = b.reserve(L.end, L.total)) return rc;
  std::vector<h2r_dev> down(n_items);
  auto* tab = reinterpret_cast<h2r_link*>(b.up.data());
  auto* devs = reinterpret_cast<h2r_dev*>(b.up.data() + L.devs);
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_reply_item& it = items[i];
    devs[i] = it.reply->h;  // (a copy: the reply's own keeps the targets of its single calls)
    h2_reply_target(&devs[i], reinterpret_cast<grdma_sge*>(it.d_slices_out), it.slices_cap, static_cast<uint8_t*>(it.d_hdr_arena), it.hdr_cap, 0, 0, 0);
    memset(devs[i].res, 0, sizeof(devs[i].res));
    tab[i].R = reinterpret_cast<h2r_dev*>(b.d + L.devs) + i;
    // behind each source parser's last deframing (a pipe step on another stream; the standalone calls share this stream)
    b.behind.push_back(it.reply->src->parser);
  }
  b.c.down.push_back({down.data(), b.d + L.devs, sizeof(h2r_dev) * n_items});
  const h2_stage framing = h2_stage_reply_links(reinterpret_cast<const h2r_link*>(b.d), n_items);
  if (int rc = b.run({h2_all(framing)})) return rc;
  g_h2_last_kernel_us = 1e3 * b.c.ms[0];
  for (uint32_t i = 0; i < n_items; i++) items[i].n_slices = h2_reply_ran(down[i].res, b.c.ms[0], items[i].out);  // (the time: the batch's, repeated)
  return 0;
}

// ---- receive flow control: the window ledger (csrc/grdma_h2_fc.h) -------------------------------------------------
struct grdma_h2_fc : h2_follow {     // (taken: the last call accounted)
  h2fc_dev* d = nullptr;
  h2fc_dev h;                      // host copy of the configuration words
  h2fc_call* d_call = nullptr;     // standalone calls
  h2_step_seq* seq = nullptr;      // the steps of the pipe, single or group, that account through it
};

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
  return h2_push_words(f->d, &h, offsetof(h2fc_dev, scratch_ev), offsetof(h2fc_dev, out), nullptr) && ok;
}

// where the calls write: the words of h2fc_dev from `out` to the state, in the host copy -> their upload
static h2_xfer h2_fc_target(grdma_h2_fc* f, grdma_sge* out, uint64_t cap, uint8_t* hdr, uint64_t hdr_cap) {
  h2fc_dev& h = f->h;
  h.out = out;
  h.cap = cap;
  h.hdr = hdr;
  h.hdr_cap = hdr_cap;
  return h2_words(f->d, &h, offsetof(h2fc_dev, out), offsetof(h2fc_dev, announced));
}
// ... uploaded at once (a pipe's)
static bool h2_fc_set_target(grdma_h2_fc* f, grdma_sge* out, uint64_t cap, uint8_t* hdr, uint64_t hdr_cap, hipStream_t st) {
  h2_fc_target(f, out, cap, hdr, hdr_cap);
  return h2_push_words(f->d, &f->h, offsetof(h2fc_dev, out), offsetof(h2fc_dev, announced), st);
}

grdma_h2_fc* grdma_h2_fc_create(grdma_h2_parser* parser, uint32_t stream_window, uint32_t conn_window, uint32_t conn_threshold,
                                uint32_t max_updates) {
  if (grdma_device_count() <= 0) return nullptr;
  if (!parser) return h2_no("h2 flow control: no parser");
  if (parser->fc) return h2_no("h2 flow control: the parser has a ledger already");
  if (stream_window == 0 || stream_window > 0x7fffffffu) return h2_no("h2 flow control: stream_window outside 1 .. 2^31 - 1");
  if (conn_window < 65535 || conn_window > 0x7fffffffu) return h2_no("h2 flow control: conn_window outside 65535 .. 2^31 - 1");
  if (conn_threshold > conn_window) return h2_no("h2 flow control: conn_threshold above conn_window");
  if (max_updates == 0 || max_updates > (1u << 24)) return h2_no("h2 flow control: max_updates outside 1 .. 2^24");
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
                  hipMemcpy(f->d, &h, sizeof(h), hipMemcpyHostToDevice) == hipSuccess;
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
  if (!f || f->seq) return;  // (the pipe's graph still runs the kernels on it: destroy the pipe first)
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);  // (standalone calls)
  if (f->parser) f->parser->fc = nullptr;
  hipFree(f->h.tab);
  hipFree(f->h.upd);
  hipFree(f->h.mark);
  hipFree(f->h.mark_pre);
  hipFree(f->d);
  hipFree(f->d_call);
  delete f;
}

// what a call on f into these targets is refused for
static const char* h2_fc_refusal(const grdma_h2_fc* f, const void* d_slices_out, uint64_t slices_cap, const void* d_hdr_arena, uint64_t hdr_cap) {
  if (!f) return "a call without ledger";
  if (f->seq) return "the ledger is attached to a pipe (its steps account)";
  if (const char* why = h2_follow_refusal(*f, "this call is accounted already", false)) return why;
  return h2_bad_target(d_slices_out, slices_cap, d_hdr_arena, hdr_cap);
}

int64_t grdma_h2_fc_account(grdma_h2_fc* f, grdma_slice* d_slices_out, uint64_t slices_cap, void* d_hdr_arena, uint64_t hdr_cap,
                            uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!out) return h2_invalid("h2 flow control", "no result array");
  if (const char* why = h2_fc_refusal(f, d_slices_out, slices_cap, d_hdr_arena, hdr_cap)) return h2_invalid("h2 flow control", why);
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  if (!h2_fc_prepare(f, f->parser->standalone_ev_cap)) return -GRDMA_ERR_HIP;
  // the stream of the standalone deframings: the call is ordered behind the one it reads
  // ... and behind the parser's last deframing by a pipe: k_h2_fc_finish reads the stream map that step may change
  if (!h2_wait_parser(hc->stream, f->parser)) return -GRDMA_ERR_HIP;
  const h2fc_call call = h2_follow_deframed(*f);
  const h2_stage ledger = h2_stage_fc(f->d, f->d_call);
  h2_call c{"grdma_h2_fc_account: a launch was rejected",
            {h2_fc_target(f, reinterpret_cast<grdma_sge*>(d_slices_out), slices_cap, static_cast<uint8_t*>(d_hdr_arena), hdr_cap),
             {f->d_call, &call, sizeof(call)}},
            {}, {h2_all(ledger)}, {h2_result(out, f->d, offsetof(h2fc_dev, res))}};
  if (int rc = h2_call_run(hc, &c)) return rc;
  h2_follow_ran(f, c.ms[0]);
  if (out[H2FC_OVERFLOW] == 2)
    return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 flow control: the call's event list overflowed, its bytes cannot be accounted");
  if (out[H2FC_OVERFLOW]) return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 flow control: more frames than max_updates, or a slice or header cap too small");
  return (int64_t)out[H2FC_SLICES];
}

// ---- the ledgers of many transports in five launches (h2_stage_fc_links) ---------------------------------------------
// The batch block of the process holds [table | one call block per item] and goes up in one copy; every item's targets
// are words of its ledger's own device block (64 bytes up per item, in the same section), as are its result words (64
// bytes down per item behind the stage).  One call at a time, as the other batch calls.
int grdma_h2_fc_account_batch(const grdma_h2_fc_item* items, uint32_t n_items, uint64_t* out) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 flow control batch", "ledger", "h2 flow control batch: a launch was rejected"};
  if (int rc = b.begin(items && out, n_items)) return rc;
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_fc_item& it = items[i];
    if (int rc = b.item(it.fc, h2_fc_refusal(it.fc, it.d_slices_out, it.slices_cap, it.d_hdr_arena, it.hdr_cap))) return rc;
  }
  for (uint32_t i = 0; i < n_items; i++)
    if (!h2_fc_prepare(items[i].fc, items[i].fc->parser->standalone_ev_cap)) return -GRDMA_ERR_HIP;
  if (int rc = b.open(sizeof(h2fc_link), sizeof(h2fc_call), n_items)) return rc;
  auto* tab = reinterpret_cast<h2fc_link*>(b.up.data());
  auto* calls = reinterpret_cast<h2fc_call*>(b.up.data() + b.blocks);
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_fc_item& it = items[i];
    grdma_h2_fc* f = it.fc;
    calls[i] = h2_follow_deframed(*f);
    tab[i] = {f->d, reinterpret_cast<const h2fc_call*>(b.d + b.blocks) + i};
    b.c.up.push_back(h2_fc_target(f, reinterpret_cast<grdma_sge*>(it.d_slices_out), it.slices_cap, static_cast<uint8_t*>(it.d_hdr_arena), it.hdr_cap));
    b.c.down.push_back(h2_result(out + 8 * (size_t)i, f->d, offsetof(h2fc_dev, res)));
    b.behind.push_back(f->parser);  // (the finish reads the stream map a pipe's deframing may change)
  }
  const h2_stage ledgers = h2_stage_fc_links(reinterpret_cast<const h2fc_link*>(b.d), n_items);
  if (int rc = b.run({h2_all(ledgers)})) return rc;
  int ok = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    h2_follow_ran(items[i].fc, b.c.ms[0]);  // (the time: the batch's, repeated)
    ok += out[8 * (size_t)i + H2FC_OVERFLOW] == 0;
  }
  return ok;
}

int grdma_h2_fc_stats(grdma_h2_fc* f, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!f || !out) return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  h2fc_dev h;
  if ((f->parser && !h2_wait_parser(hc->stream, f->parser)) || !h2_read(&h, f->d, sizeof(h))) return -GRDMA_ERR_HIP;
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

// ---- send flow control: the peer's windows and the framer under them (csrc/grdma_h2_sw.h) -------------------------------
struct grdma_h2_sw : h2_follow {        // (taken: the last call taken in; at creation: the calls before it)
  h2sw_dev* d = nullptr;
  h2sw_dev h;                         // host copy of the configuration words
  h2sw_call* d_call = nullptr;
  grdma_h2_msg_dev* d_msgs = nullptr; // H2_FRAME_ONE_MAX
  uint64_t* d_prog = nullptr;         // progress in [0, MAX), out [MAX, 2 MAX)
  struct grdma_h2_reply* reply = nullptr;  // the reply framer whose queue waits under these windows (csrc/grdma_h2_wr.h)
  bool reply_gone = false;                 // ... has been destroyed: every call but destroy is refused
};

grdma_h2_sw* grdma_h2_sw_create(grdma_h2_parser* parser, uint32_t initial_window, uint32_t conn_window, uint32_t peer_max_frame) {
  if (grdma_device_count() <= 0) return nullptr;
  if (!parser) return h2_no("h2 send windows: no parser");
  if (parser->sw) return h2_no("h2 send windows: the parser has send windows already");
  if (initial_window > 0x7fffffffu || conn_window > 0x7fffffffu) return h2_no("h2 send windows: a window above 2^31 - 1");
  if (peer_max_frame < 16384 || peer_max_frame > 16777215) return h2_no("h2 send windows: peer_max_frame outside 16384 .. 2^24 - 1");
  grdma_h2_sw* s = new grdma_h2_sw();
  s->parser = parser;
  s->taken = parser->standalone_calls;
  memset(&s->h, 0, sizeof(s->h));
  h2sw_dev& h = s->h;
  h.gp = parser->d;
  h.tab_mask = parser->slots - 1;
  h.conn = (long long)conn_window;
  h.iws = initial_window;
  h.pmf = peer_max_frame;
  const size_t tab_bytes = sizeof(h2sw_slot) * parser->slots;
  const bool ok = hipMalloc((void**)&s->d, sizeof(h2sw_dev)) == hipSuccess &&
                  hipMalloc((void**)&h.tabs[0], tab_bytes) == hipSuccess && hipMalloc((void**)&h.tabs[1], tab_bytes) == hipSuccess &&
                  hipMalloc((void**)&h.pieces, sizeof(h2sw_piece) * H2_FRAME_ONE_MAX) == hipSuccess &&
                  hipMalloc((void**)&h.pos, sizeof(grdma_h2_msg_pos) * H2_FRAME_ONE_MAX) == hipSuccess &&
                  hipMalloc((void**)&h.slot_of, sizeof(uint32_t) * H2_FRAME_ONE_MAX) == hipSuccess &&
                  hipMalloc((void**)&s->d_msgs, sizeof(grdma_h2_msg_dev) * H2_FRAME_ONE_MAX) == hipSuccess &&
                  hipMalloc((void**)&s->d_prog, sizeof(uint64_t) * 2 * H2_FRAME_ONE_MAX) == hipSuccess &&
                  hipMalloc((void**)&s->d_call, sizeof(h2sw_call)) == hipSuccess &&
                  hipMemset(h.tabs[0], 0, tab_bytes) == hipSuccess && hipMemset(h.tabs[1], 0, tab_bytes) == hipSuccess;
  h.msgs = s->d_msgs;
  h.prog_in = s->d_prog;
  h.prog_out = s->d_prog ? s->d_prog + H2_FRAME_ONE_MAX : nullptr;
  parser->sw = s;
  if (!ok || hipMemcpy(s->d, &h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    grdma_h2_sw_destroy(s);
    grdma_fail_msg(GRDMA_ERR_HIP, "h2 send windows: device allocation failed");
    return nullptr;
  }
  return s;
}

void grdma_h2_sw_destroy(grdma_h2_sw* s) {
  if (!s) return;
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);  // (standalone calls)
  if (s->parser) s->parser->sw = nullptr;
  if (s->reply) s->reply->sw = nullptr;  // (the reply outlives its windows as a husk: every call on it is refused)
  hipFree(s->h.tabs[0]);
  hipFree(s->h.tabs[1]);
  hipFree(s->h.pieces);
  hipFree(s->h.pos);
  hipFree(s->h.slot_of);
  hipFree(s->d_msgs);
  hipFree(s->d_prog);
  hipFree(s->d_call);
  hipFree(s->d);
  delete s;
}

// what every call on s but destroy is refused for
static const char* h2_sw_gone(const grdma_h2_sw* s) {
  if (!s) return "a call without send windows";
  if (!s->parser) return "the parser is gone";
  if (s->reply_gone) return "the reply framer whose queue waited under them is gone";
  return nullptr;
}
static const char* h2_sw_intake_refusal(const grdma_h2_sw* s) {
  if (const char* why = h2_sw_gone(s)) return why;
  return h2_follow_refusal(*s, "this call is taken in already", true);
}
// (the single call's arguments are an item of the batch)
static const char* h2_sw_frame_refusal(const grdma_h2_sw_frame_item& it) {
  if (const char* why = h2_sw_gone(it.sw)) return why;
  if (!it.msgs || !it.progress) return "no message table or progress";
  if (it.nmsgs == 0 || it.nmsgs > H2_FRAME_ONE_MAX) return "1 .. 4096 messages a call";
  if (it.max_frame == 0 || it.max_frame >= (1u << 24)) return "max_frame outside 1 .. 2^24 - 1";
  if (const char* why = h2_bad_target(it.d_slices_out, it.slices_cap, it.d_hdr_arena, it.hdr_cap)) return why;
  for (uint64_t m = 0; m < it.nmsgs; m++) {
    if (it.msgs[m].len >= (1ull << 32)) return "a message of 2^32 bytes or more";
    if (it.progress[m] >= 5 + it.msgs[m].len) return "a message with nothing left to send";
  }
  return nullptr;
}
// The framing call of an item: the words of h2sw_dev from `msgs` to the state in the host copy, and its transfers added
// to c -- the table (tab: it.msgs in the device's form), the progress and the words up into the send windows' own device
// memory, the result words (to res) and the progress behind the call (to after) down from there.
static void h2_sw_frame_transfers(h2_call* c, const grdma_h2_sw_frame_item& it, const grdma_h2_msg_dev* tab, uint64_t* res, uint64_t* after) {
  grdma_h2_sw* s = it.sw;
  h2sw_dev& h = s->h;
  h.nmsgs = it.nmsgs;
  h.max_frame = it.max_frame;
  h.out = reinterpret_cast<grdma_sge*>(it.d_slices_out);
  h.cap = it.slices_cap;
  h.hdr = static_cast<uint8_t*>(it.d_hdr_arena);
  h.hdr_cap = it.hdr_cap;
  c->up.push_back({s->d_msgs, tab, sizeof(grdma_h2_msg_dev) * it.nmsgs});
  c->up.push_back({s->d_prog, it.progress, sizeof(uint64_t) * it.nmsgs});
  c->up.push_back(h2_words(s->d, &h, offsetof(h2sw_dev, msgs), offsetof(h2sw_dev, conn)));
  c->down.push_back(h2_result(res, s->d, offsetof(h2sw_dev, fres)));
  c->down.push_back({after, s->d_prog + H2_FRAME_ONE_MAX, sizeof(uint64_t) * it.nmsgs});
}
// behind a framing call that ran -> whether the item's frames stand
static bool h2_sw_frame_ran(const grdma_h2_sw_frame_item& it, float ms, const uint64_t* res, const uint64_t* after) {
  it.sw->last_ms = ms;
  if (res[H2SW_F_OVERFLOW]) return false;  // (nothing was written, no window moved: progress stays as it is)
  for (uint64_t m = 0; m < it.nmsgs; m++) it.progress[m] = after[m];
  return true;
}

int64_t grdma_h2_sw_intake(grdma_h2_sw* s, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!out) return h2_invalid("h2 send windows", "no result array");
  if (const char* why = h2_sw_intake_refusal(s)) return h2_invalid("h2 send windows", why);
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  // the stream of the standalone deframings: the call is ordered behind the one it reads, and behind the parser's last
  // deframing by a pipe (the intake reads the stream map that step may change)
  if (!h2_wait_parser(hc->stream, s->parser)) return -GRDMA_ERR_HIP;
  const h2sw_call call = h2_follow_deframed(*s);
  const h2_stage intake = h2_stage_sw_intake(s->d, s->d_call);
  h2_call c{"grdma_h2_sw_intake: a launch was rejected",
            {{s->d_call, &call, sizeof(call)}}, {}, {h2_all(intake)}, {h2_result(out, s->d, offsetof(h2sw_dev, res))}};
  if (int rc = h2_call_run(hc, &c)) return rc;
  h2_follow_ran(s, c.ms[0]);
  if (out[H2SW_I_OVERFLOW])
    return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 send windows: the call's event list overflowed, its frames cannot be taken in");
  return (int64_t)out[H2SW_I_UPDATES];
}

int64_t grdma_h2_sw_frame(grdma_h2_sw* s, const grdma_h2_msg* msgs, uint64_t* progress, uint64_t n, uint32_t max_frame,
                          grdma_slice* d_slices_out, uint64_t slices_cap, void* d_hdr_arena, uint64_t hdr_cap, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!out) return h2_invalid("h2 send windows", "no result array");
  const grdma_h2_sw_frame_item it{s, msgs, progress, n, max_frame, 0, d_slices_out, slices_cap, d_hdr_arena, hdr_cap};
  if (const char* why = h2_sw_frame_refusal(it)) return h2_invalid("h2 send windows", why);
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  if (!h2_wait_parser(hc->stream, s->parser)) return -GRDMA_ERR_HIP;  // (the plan looks streams up in the map)
  const std::vector<grdma_h2_msg_dev> tab = h2_msg_table(msgs, n);
  const h2_stage framing = h2_stage_sw_frame(s->d);
  std::vector<uint64_t> after(n);
  h2_call c{"grdma_h2_sw_frame: a launch was rejected", {}, {}, {h2_all(framing)}, {}};
  h2_sw_frame_transfers(&c, it, tab.data(), out, after.data());
  if (int rc = h2_call_run(hc, &c)) return rc;
  if (!h2_sw_frame_ran(it, c.ms[0], out, after.data())) return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 send windows: a slice or header cap too small");
  return (int64_t)out[H2SW_F_SLICES];
}

int grdma_h2_sw_windows(grdma_h2_sw* s, const uint32_t* ids, uint32_t n, int64_t* out) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!s || (n && (!ids || !out))) return -GRDMA_ERR_INVALID;
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  h2sw_dev h;
  const uint32_t slots = s->h.tab_mask + 1;
  std::vector<h2sw_slot> tab(slots);
  if (!h2_read(&h, s->d, sizeof(h)) || !h2_read(tab.data(), h.tabs[h.cur & 1u], sizeof(h2sw_slot) * slots)) return -GRDMA_ERR_HIP;
  for (uint32_t i = 0; i < n; i++) {
    if (ids[i] == 0) {
      out[i] = h.conn;
      continue;
    }
    int64_t delta = 0;  // (a missing entry)
    uint32_t t = (ids[i] >> 1) & h.tab_mask;
    for (uint32_t probe = 0; probe < slots && tab[t].key != 0; probe++, t = (t + 1) & h.tab_mask)
      if (tab[t].key == ids[i]) {
        delta = tab[t].delta;
        break;
      }
    out[i] = (int64_t)h.iws + delta;
  }
  return 0;
}

int grdma_h2_sw_stats(grdma_h2_sw* s, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!s || !out) return -GRDMA_ERR_INVALID;
  h2sw_dev h;
  if (!h2_read(&h, s->d, sizeof(h))) return -GRDMA_ERR_HIP;
  out[0] = h.st_intakes;
  out[1] = h.st_updates;
  out[2] = h.st_settings;
  out[3] = h.st_violations | (h.lost ? 1ull << 63 : 0);
  out[4] = h.st_frame_calls;
  out[5] = h.st_sent;
  out[6] = (uint64_t)h.iws | ((uint64_t)h.pmf << 32);
  out[7] = (uint64_t)(s->last_ms * 1e6f);
  return 0;
}

// ---- the send windows of many transports: an intake in three launches, a framing in two (h2_stage_sw_*_links) --------
// The batch block of the process holds [table | one call block per item] (the ledger batch's shape; a framing has no
// call blocks) and goes up in one copy.  An item's message table, progress and configuration words go up into its own
// grdma_h2_sw's device memory, and its result words and progress come down from there.  One call at a time, as the other
// batch calls.
int grdma_h2_sw_intake_batch(grdma_h2_sw* const* sws, uint32_t n_items, uint64_t* out) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 send windows batch", "send windows", "h2 send windows batch: a launch was rejected"};
  if (int rc = b.begin(sws && out, n_items)) return rc;
  for (uint32_t i = 0; i < n_items; i++)
    if (int rc = b.item(sws[i], h2_sw_intake_refusal(sws[i]))) return rc;
  if (int rc = b.open(sizeof(h2sw_link), sizeof(h2sw_call), n_items)) return rc;
  auto* tab = reinterpret_cast<h2sw_link*>(b.up.data());
  auto* calls = reinterpret_cast<h2sw_call*>(b.up.data() + b.blocks);
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_sw* s = sws[i];
    calls[i] = h2_follow_deframed(*s);
    tab[i] = {s->d, reinterpret_cast<const h2sw_call*>(b.d + b.blocks) + i};
    b.c.down.push_back(h2_result(out + 8 * (size_t)i, s->d, offsetof(h2sw_dev, res)));
    b.behind.push_back(s->parser);  // (the intake reads the stream map a pipe's deframing may change)
  }
  const h2_stage intake = h2_stage_sw_intake_links(reinterpret_cast<const h2sw_link*>(b.d), n_items);
  if (int rc = b.run({h2_all(intake)})) return rc;
  int ok = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    h2_follow_ran(sws[i], b.c.ms[0]);  // (the time: the batch's, repeated)
    ok += out[8 * (size_t)i + H2SW_I_OVERFLOW] == 0;
  }
  return ok;
}

int grdma_h2_sw_frame_batch(const grdma_h2_sw_frame_item* items, uint32_t n_items, uint64_t* out) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 send windows batch", "send windows", "h2 send windows batch: a launch was rejected"};
  if (int rc = b.begin(items && out, n_items)) return rc;
  uint64_t n_msgs = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    if (int rc = b.item(items[i].sw, h2_sw_frame_refusal(items[i]))) return rc;
    n_msgs += items[i].nmsgs;
  }
  if (int rc = b.open(sizeof(h2sw_link), 0, n_items)) return rc;  // (a framing has no call blocks)
  auto* tab = reinterpret_cast<h2sw_link*>(b.up.data());
  // every item's message table in the device's form and its progress behind the call: [at[i], at[i] + nmsgs)
  std::vector<grdma_h2_msg_dev> msgs(n_msgs);
  std::vector<uint64_t> after(n_msgs), at(n_items);
  uint64_t off = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_sw_frame_item& it = items[i];
    at[i] = off;
    h2_msg_rows(it.msgs, it.nmsgs, msgs.data() + off);
    tab[i] = {it.sw->d, nullptr};
    h2_sw_frame_transfers(&b.c, it, msgs.data() + off, out + 8 * (size_t)i, after.data() + off);
    b.behind.push_back(it.sw->parser);  // (the plan looks streams up in the map)
    off += it.nmsgs;
  }
  const h2_stage framing = h2_stage_sw_frame_links(reinterpret_cast<const h2sw_link*>(b.d), n_items);
  if (int rc = b.run({h2_all(framing)})) return rc;
  int ok = 0;
  for (uint32_t i = 0; i < n_items; i++) ok += h2_sw_frame_ran(items[i], b.c.ms[0], out + 8 * (size_t)i, after.data() + at[i]);  // (the time: the batch's, repeated)
  return ok;
}

// ---- replies under the peer's windows: the queue in device memory, the windowed framer over it (csrc/grdma_h2_wr.h) -----
// The queue's device block holds the call: the host pushes the three call words, and a LOCAL copy of the send windows'
// framing words (targets, frame size) -- the mirror grdma_h2_sw_frame pushes from stays as that call left it.  Where the
// plan's table lies and how many messages it holds is written on the device (k_h2_wr_queue).
static void h2_wr_free(grdma_h2_reply* r) {
  if (!r->wr.max_pending) return;  // (never attached)
  if (r->sw) {
    r->sw->reply = nullptr;
    r->sw->reply_gone = true;  // (what waited in the queue is gone with it: the windows refuse every call but destroy)
  }
  for (int t = 0; t < 2; t++) {
    hipFree(r->wr.msgs[t]);
    hipFree(r->wr.prog[t]);
    hipFree(r->wr.rank[t]);
  }
  hipFree(r->d_wr);
  memset(&r->wr, 0, sizeof(r->wr));
  r->d_wr = nullptr;
  r->sw = nullptr;
}

int grdma_h2_reply_attach_windows(grdma_h2_reply* r, grdma_h2_sw* s, uint32_t max_pending) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!r || !s) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 windowed reply: a reply and send windows");
  if (max_pending == 0 || max_pending > H2_FRAME_ONE_MAX) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 windowed reply: max_pending outside 1 .. 4096");
  if (r->seq) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 windowed reply: the reply is bound to a reply pipe");
  if (r->src->attached) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 windowed reply: the source assembler is attached to a pipe");
  if (r->d_wr) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 windowed reply: the reply has send windows attached already");
  if (s->reply || s->reply_gone) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 windowed reply: the send windows are attached to a reply already");
  if (!s->parser) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 windowed reply: the send windows' parser is gone");
  h2_host_ctx* hc = h2_ctx();
  if (!hc || hipStreamSynchronize(hc->stream) != hipSuccess) return -GRDMA_ERR_HIP;
  h2wr_dev& w = r->wr;
  memset(&w, 0, sizeof(w));
  w.R = r->d;
  w.F = s->d;
  w.max_pending = max_pending;
  bool ok = hipMalloc((void**)&r->d_wr, sizeof(h2wr_dev)) == hipSuccess;
  for (int t = 0; t < 2 && ok; t++)
    ok = hipMalloc((void**)&w.msgs[t], sizeof(grdma_h2_msg_dev) * max_pending) == hipSuccess &&
         hipMalloc((void**)&w.prog[t], sizeof(uint64_t) * max_pending) == hipSuccess &&
         hipMalloc((void**)&w.rank[t], sizeof(uint64_t) * max_pending) == hipSuccess;
  ok = ok && hipMemcpy(r->d_wr, &w, sizeof(w), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    h2_wr_free(r);
    return grdma_fail_msg(GRDMA_ERR_HIP, "h2 windowed reply: device allocation failed");
  }
  r->sw = s;
  s->reply = r;
  r->taken = r->attached_at = r->src->calls;
  r->pending = 0;
  return 0;
}

// what a call on r is refused for, the targets included
static const char* h2_wr_refusal(const grdma_h2_reply* r, uint32_t flags, const void* d_slices_out, uint64_t slices_cap,
                                 const void* d_hdr_arena, uint64_t hdr_cap) {
  if (!r) return "no reply";
  if (!r->d_wr) return "the reply has no send windows attached";
  if (!r->sw) return "the send windows are gone";
  if (!r->sw->parser) return "the send windows' parser is gone";
  if (r->seq || r->src->attached) return "a reply or source assembler bound to a pipe";
  if (flags & ~(uint32_t)GRDMA_H2_WR_PENDING_ONLY) return "unknown flags";
  if (const char* why = h2_bad_target(d_slices_out, slices_cap, d_hdr_arena, hdr_cap)) return why;
  if (r->src->calls == r->attached_at && r->pending == 0) return "no source call yet and nothing waits";
  return nullptr;
}

// the call words of r's queue for one call, in its host copy -> whether the source's last call is to be taken
static bool h2_wr_call_words(grdma_h2_reply* r, uint32_t flags) {
  const uint64_t calls = r->src->calls;
  const bool is_new = calls > r->taken;
  const bool take = is_new && !(flags & GRDMA_H2_WR_PENDING_ONLY);
  r->wr.take = take ? 1 : 0;
  r->wr.untaken = (is_new && !take) ? 1 : 0;
  r->wr.lost_now = calls > r->taken + 1 ? 1 : 0;
  return take;
}

// A call of r, its transfers added to c: the call words up into the queue, the send windows' framing words up from
// *words -- a LOCAL copy of their mirror with the call's targets -- and the queue's result block down to res.
// -> whether the source's last call is to be taken
static bool h2_wr_transfers(h2_call* c, grdma_h2_reply* r, uint32_t flags, grdma_slice* d_slices_out, uint64_t slices_cap, void* d_hdr_arena,
                            uint64_t hdr_cap, h2sw_dev* words, uint64_t* res) {
  const bool take = h2_wr_call_words(r, flags);
  h2sw_dev& h = *words = r->sw->h;
  h.msgs = r->wr.msgs[0];   // (k_h2_wr_queue names the table and the count)
  h.prog_in = r->wr.prog[0];
  h.nmsgs = 0;
  h.max_frame = r->h.max_frame;
  h.out = reinterpret_cast<grdma_sge*>(d_slices_out);
  h.cap = slices_cap;
  h.hdr = static_cast<uint8_t*>(d_hdr_arena);
  h.hdr_cap = hdr_cap;
  c->up.push_back(h2_words(r->d_wr, &r->wr, offsetof(h2wr_dev, take), offsetof(h2wr_dev, n_tab)));
  c->up.push_back(h2_words(r->sw->d, words, offsetof(h2sw_dev, msgs), offsetof(h2sw_dev, conn)));
  c->down.push_back(h2_result(res, r->d_wr, offsetof(h2wr_dev, res), 16));
  return take;
}

// behind a call of r that ran: what the host keeps of it, and its result block to the caller -> whether it stands
static bool h2_wr_ran(grdma_h2_reply* r, bool take, const uint64_t res[16], float ms, uint64_t out[16]) {
  for (int i = 0; i < 16; i++) out[i] = res[i];
  out[H2WR_US] = (uint64_t)(ms * 1e3f);
  const uint64_t calls = r->src->calls;
  if (calls > r->taken + 1) r->taken = calls - 1;  // (lost: the flag is the device's and sticky)
  r->sw->last_ms = ms;
  if (res[H2WR_OVERFLOW]) return false;  // (the queue stands, the source call is not taken)
  if (take) r->taken = calls;
  r->pending = res[H2WR_PENDING];
  return true;
}

int64_t grdma_h2_reply_frame_windowed(grdma_h2_reply* r, uint32_t flags, grdma_slice* d_slices_out, uint64_t slices_cap,
                                      void* d_hdr_arena, uint64_t hdr_cap, uint64_t out[16]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!out) return h2_invalid("h2 windowed reply", "no result array");
  if (const char* why = h2_wr_refusal(r, flags, d_slices_out, slices_cap, d_hdr_arena, hdr_cap)) return h2_invalid("h2 windowed reply", why);
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  // behind the source parser's last deframing (the descriptors) and the last one of the send windows' parser (the map)
  if (!h2_wait_parser(hc->stream, r->src->parser) || !h2_wait_parser(hc->stream, r->sw->parser)) return -GRDMA_ERR_HIP;
  const h2_stage framing = h2_stage_wr_frame(r->d_wr, r->sw->d);
  h2sw_dev words;
  uint64_t res[16];
  h2_call c{"grdma_h2_reply_frame_windowed: a launch was rejected", {}, {}, {h2_all(framing)}, {}};
  const bool take = h2_wr_transfers(&c, r, flags, d_slices_out, slices_cap, d_hdr_arena, hdr_cap, &words, res);
  if (int rc = h2_call_run(hc, &c)) return rc;
  if (h2_wr_ran(r, take, res, c.ms[0], out)) return (int64_t)res[H2WR_SLICES];
  if (res[H2WR_OVERFLOW] == 2) return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 windowed reply: more entries than max_pending");
  return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 windowed reply: a slice or header cap too small, a skipped source call or more descriptors than max_messages");
}

int64_t grdma_h2_reply_pending(grdma_h2_reply* r, uint64_t* out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!r || !r->d_wr || (!out && cap)) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 windowed reply: no reply, no send windows attached or no array");
  h2wr_dev w;
  if (!h2_read(&w, r->d_wr, sizeof(w))) return -GRDMA_ERR_HIP;
  const uint64_t n = w.nq < w.max_pending ? w.nq : w.max_pending;
  std::vector<grdma_h2_msg_dev> msgs(n ? n : 1);
  std::vector<uint64_t> prog(n ? n : 1);
  if (n && (!h2_read(msgs.data(), w.msgs[w.cur & 1u], sizeof(grdma_h2_msg_dev) * n) || !h2_read(prog.data(), w.prog[w.cur & 1u], sizeof(uint64_t) * n)))
    return -GRDMA_ERR_HIP;
  uint64_t k = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (prog[i] >= 5 + msgs[i].len) continue;  // (finished: the next call's compaction drops it)
    if (k < cap) {
      out[3 * k] = msgs[i].stream_id;
      out[3 * k + 1] = msgs[i].len;
      out[3 * k + 2] = prog[i];
    }
    k++;
  }
  return (int64_t)k;
}

// ---- the windowed replies of many transports in four launches (h2_stage_wr_frame_links) -------------------------------
// The batch block of the process holds [the queues' table | the send windows' table] (the ledger batch's layout: the
// second table where that one has its call blocks) and goes up in one copy; an item's call words and framing words go up
// into its own queue's and send windows' device memory, its result block comes down from its queue.
int grdma_h2_reply_frame_windowed_batch(grdma_h2_wr_item* items, uint32_t n_items) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 windowed reply batch", "reply", "h2 windowed reply batch: a launch was rejected"};
  if (int rc = b.begin(items, n_items)) return rc;
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_wr_item& it = items[i];
    if (int rc = b.item(it.reply, h2_wr_refusal(it.reply, it.flags, it.d_slices_out, it.slices_cap, it.d_hdr_arena, it.hdr_cap))) return rc;
    for (uint32_t k = 0; k < i; k++)
      if (items[k].reply->src == it.reply->src) return h2_invalid(b.who, "two replies of one source assembler");
  }
  if (int rc = b.open(sizeof(h2wr_link), sizeof(h2sw_link), n_items)) return rc;
  auto* tab = reinterpret_cast<h2wr_link*>(b.up.data());
  auto* sw_tab = reinterpret_cast<h2sw_link*>(b.up.data() + b.blocks);
  std::vector<h2sw_dev> words(n_items);
  std::vector<uint64_t> res(16 * (size_t)n_items);
  std::vector<char> take(n_items);
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_wr_item& it = items[i];
    grdma_h2_reply* r = it.reply;
    take[i] = h2_wr_transfers(&b.c, r, it.flags, it.d_slices_out, it.slices_cap, it.d_hdr_arena, it.hdr_cap, &words[i], res.data() + 16 * (size_t)i);
    tab[i].W = r->d_wr;
    sw_tab[i] = {r->sw->d, nullptr};
    b.behind.push_back(r->src->parser);  // (the descriptors)
    b.behind.push_back(r->sw->parser);   // (the map)
  }
  const h2_stage framing = h2_stage_wr_frame_links(reinterpret_cast<const h2wr_link*>(b.d), reinterpret_cast<const h2sw_link*>(b.d + b.blocks), n_items);
  if (int rc = b.run({h2_all(framing)})) return rc;
  g_h2_last_kernel_us = 1e3 * b.c.ms[0];
  int ok = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    grdma_h2_wr_item& it = items[i];
    const uint64_t* rs = res.data() + 16 * (size_t)i;
    const bool stands = h2_wr_ran(it.reply, take[i] != 0, rs, b.c.ms[0], it.out);  // (the time: the batch's, repeated)
    it.n_slices = stands ? (int64_t)rs[H2WR_SLICES] : -(int64_t)GRDMA_ERR_CAPACITY;
    ok += stands;
  }
  return ok;
}

// ---- control replies: SETTINGS ACK, PING ACK, RST_STREAM from a deframing's events (csrc/grdma_h2_ctl.h) ---------------
struct grdma_h2_ctl : h2_follow {  // (taken: the last call taken in; at creation: the calls before it)
  h2ctl_dev* d = nullptr;
  h2ctl_call* d_call = nullptr;
};

struct grdma_h2_hpack : h2_follow {  // (csrc/grdma_h2_hpack.h; its calls stand behind the control replies')
  h2hp_dev* d = nullptr;
  h2hp_call* d_call = nullptr;
  uint8_t* d_carry = nullptr;
  // a call's scratch, grown between the call's two steps
  uint8_t* d_stage = nullptr;
  uint64_t stage_cap = 0;
  h2hp_rec* d_recs = nullptr;
  uint64_t recs_cap = 0;
  h2hp_rec* d_outs = nullptr;
  uint64_t outs_cap = 0;
  h2hp_item* d_items = nullptr;
  uint64_t items_cap = 0;
  h2hp_blk* d_blks = nullptr;
  uint64_t blks_cap = 0;
};

static void h2_followers_parser_gone(grdma_h2_parser* p) {
  h2_follow* const followers[4] = {p->fc, p->sw, p->ctl, p->hpack};
  for (h2_follow* f : followers)
    if (f) h2_follow_parser_gone(f);
}

grdma_h2_ctl* grdma_h2_ctl_create(grdma_h2_parser* parser, uint32_t max_replies) {
  if (grdma_device_count() <= 0) return nullptr;
  if (!parser) return h2_no("h2 control replies: no parser");
  if (parser->ctl) return h2_no("h2 control replies: the parser has a control-reply writer already");
  if (max_replies == 0 || max_replies > (1u << 24)) return h2_no("h2 control replies: max_replies outside 1 .. 2^24");
  grdma_h2_ctl* w = new grdma_h2_ctl();
  w->parser = parser;
  w->taken = parser->standalone_calls;
  parser->ctl = w;
  const uint64_t max64 = max_replies;
  if (hipMalloc((void**)&w->d, sizeof(h2ctl_dev)) != hipSuccess || hipMalloc((void**)&w->d_call, sizeof(h2ctl_call)) != hipSuccess ||
      hipMemset(w->d, 0, sizeof(h2ctl_dev)) != hipSuccess ||
      hipMemcpy(reinterpret_cast<uint8_t*>(w->d) + offsetof(h2ctl_dev, max_replies), &max64, sizeof(max64), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    grdma_h2_ctl_destroy(w);
    grdma_fail_msg(GRDMA_ERR_HIP, "h2 control replies: device allocation failed");
    return nullptr;
  }
  return w;
}

void grdma_h2_ctl_destroy(grdma_h2_ctl* w) {
  if (!w) return;
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);  // (standalone calls)
  if (w->parser) w->parser->ctl = nullptr;
  hipFree(w->d_call);
  hipFree(w->d);
  delete w;
}

// what a call of an item (the single call's arguments are one) is refused for
static const char* h2_ctl_refusal(const grdma_h2_ctl_item& it) {
  if (!it.ctl) return "a call without writer";
  if (const char* why = h2_follow_refusal(*it.ctl, "this call is taken in already", true)) return why;
  return h2_bad_target(it.d_slices_out, it.slices_cap, it.d_hdr_arena, it.hdr_cap);
}
// where an item's call writes: the leading words of its writer's device block
struct h2ctl_target { grdma_sge* out; uint64_t cap; uint8_t* hdr; uint64_t hdr_cap; };
static_assert(offsetof(h2ctl_dev, out) == 0 && offsetof(h2ctl_dev, max_replies) == sizeof(h2ctl_target), "a call's target leads the block");
static h2ctl_target h2_ctl_target(const grdma_h2_ctl_item& it) {
  return {reinterpret_cast<grdma_sge*>(it.d_slices_out), it.slices_cap, static_cast<uint8_t*>(it.d_hdr_arena), it.hdr_cap};
}
// behind a call of w that ran, res its result words -> whether its frames stand
static bool h2_ctl_ran(grdma_h2_ctl* w, float ms, const uint64_t* res) {
  // (a cap overflow, 1: nothing was written or committed, the call is not taken and may be repeated)
  h2_follow_ran(w, ms, res[H2CTL_OVERFLOW] != 1);
  return res[H2CTL_OVERFLOW] == 0;
}

int64_t grdma_h2_ctl_reply(grdma_h2_ctl* w, grdma_slice* d_slices_out, uint64_t slices_cap, void* d_hdr_arena, uint64_t hdr_cap,
                           uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!out) return h2_invalid("h2 control replies", "no result array");
  const grdma_h2_ctl_item it{w, d_slices_out, slices_cap, d_hdr_arena, hdr_cap};
  if (const char* why = h2_ctl_refusal(it)) return h2_invalid("h2 control replies", why);
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  // the stream of the standalone deframings: the call is ordered behind the one it reads
  if (!h2_wait_parser(hc->stream, w->parser)) return -GRDMA_ERR_HIP;
  const h2ctl_call call = h2_follow_deframed(*w);
  const h2ctl_target target = h2_ctl_target(it);
  const h2_stage stage = h2_stage_ctl(w->d, w->d_call);
  h2_call c{"grdma_h2_ctl_reply: a launch was rejected",
            {{w->d_call, &call, sizeof(call)}, {w->d, &target, sizeof(target)}}, {}, {h2_all(stage)},
            {h2_result(out, w->d, offsetof(h2ctl_dev, res))}};
  if (int rc = h2_call_run(hc, &c)) return rc;
  if (h2_ctl_ran(w, c.ms[0], out)) return (int64_t)out[H2CTL_SLICES];
  if (out[H2CTL_OVERFLOW] == 1)
    return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 control replies: more replies than max_replies, or a slice or header cap too small");
  return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 control replies: the call's event list overflowed, its frames cannot be answered");
}

int grdma_h2_ctl_peer(grdma_h2_ctl* w, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w || !out) return -GRDMA_ERR_INVALID;
  if (!h2_read(out, reinterpret_cast<const uint8_t*>(w->d) + offsetof(h2ctl_dev, peer), 8 * sizeof(uint64_t))) return -GRDMA_ERR_HIP;
  return 0;
}

int grdma_h2_ctl_stats(grdma_h2_ctl* w, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w || !out) return -GRDMA_ERR_INVALID;
  uint64_t st[5];
  uint32_t lost[2];
  if (!h2_read(st, reinterpret_cast<const uint8_t*>(w->d) + offsetof(h2ctl_dev, st_calls), sizeof(st)) ||
      !h2_read(lost, reinterpret_cast<const uint8_t*>(w->d) + offsetof(h2ctl_dev, lost), sizeof(lost)))
    return -GRDMA_ERR_HIP;
  for (int i = 0; i < 5; i++) out[i] = st[i];  // calls, SETTINGS ACKs, PING ACKs, RST_STREAMs, wire bytes
  out[5] = 0;
  out[6] = lost[0] ? 1 : 0;
  out[7] = (uint64_t)(w->last_ms * 1e6f);
  return 0;
}

// The writers of many transports in the same four launches (h2_stage_ctl_links).  The batch block of the process holds
// [table | one call block per item] (the ledger batch's shape) and goes up in one copy; an item's targets are the leading
// words of its writer's own device block, its result words come down from there.  One call at a time, as the other batch
// calls.
int grdma_h2_ctl_reply_batch(const grdma_h2_ctl_item* items, uint32_t n_items, uint64_t* out) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 control replies batch", "writer", "h2 control replies batch: a launch was rejected"};
  if (int rc = b.begin(items && out, n_items)) return rc;
  for (uint32_t i = 0; i < n_items; i++)
    if (int rc = b.item(items[i].ctl, h2_ctl_refusal(items[i]))) return rc;
  if (int rc = b.open(sizeof(h2ctl_link), sizeof(h2ctl_call), n_items)) return rc;
  auto* tab = reinterpret_cast<h2ctl_link*>(b.up.data());
  auto* calls = reinterpret_cast<h2ctl_call*>(b.up.data() + b.blocks);
  std::vector<h2ctl_target> targets(n_items);
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_ctl* w = items[i].ctl;
    calls[i] = h2_follow_deframed(*w);
    tab[i] = {w->d, reinterpret_cast<const h2ctl_call*>(b.d + b.blocks) + i};
    targets[i] = h2_ctl_target(items[i]);
    b.c.up.push_back({w->d, &targets[i], sizeof(h2ctl_target)});
    b.c.down.push_back(h2_result(out + 8 * (size_t)i, w->d, offsetof(h2ctl_dev, res)));
    b.behind.push_back(w->parser);
  }
  const h2_stage stage = h2_stage_ctl_links(reinterpret_cast<const h2ctl_link*>(b.d), n_items);
  if (int rc = b.run({h2_all(stage)})) return rc;
  int ok = 0;
  for (uint32_t i = 0; i < n_items; i++) ok += h2_ctl_ran(items[i].ctl, b.c.ms[0], out + 8 * (size_t)i);  // (the time: the batch's, repeated)
  return ok;
}

// ---- header blocks: HPACK on the device (csrc/grdma_h2_hpack.h) ----------------------------------------------------------
// The decoder follows the parser's standalone deframings as the control-reply writer does.  A call has two steps on the
// stream of the calls: the gather, whose totals come down, and -- the staging buffer and the record tables sized by
// them -- the other stages.
struct h2hp_target { h2hp_block_out* blocks; uint64_t blocks_cap; h2hp_field_out* fields; uint64_t fields_cap; uint8_t* strings; uint64_t strings_cap; };
struct h2hp_scratch { uint8_t* stage; uint64_t stage_cap; h2hp_rec* recs; uint64_t recs_cap; h2hp_rec* outs; uint64_t outs_cap;
                      h2hp_item* items; h2hp_blk* blks; uint64_t items_cap; };
struct h2hp_config { uint8_t* carry_buf; uint64_t max_block; uint32_t setting, pad0; };
static_assert(offsetof(h2hp_dev, blocks) == 0 && offsetof(h2hp_dev, stage) == sizeof(h2hp_target) &&
              offsetof(h2hp_dev, carry_buf) == sizeof(h2hp_target) + sizeof(h2hp_scratch) &&
              offsetof(h2hp_dev, carry) == offsetof(h2hp_dev, carry_buf) + sizeof(h2hp_config),
              "a call's target, its scratch and the configuration lead the block");
static_assert(sizeof(h2hp_block_out) == sizeof(grdma_h2_header_block) && sizeof(h2hp_field_out) == sizeof(grdma_h2_header_field), "layout");
static_assert(H2HP_F_FAILED == GRDMA_H2_HPACK_FAILED && H2HP_F_LOST == GRDMA_H2_HPACK_LOST && H2HP_F_OPEN == GRDMA_H2_HPACK_OPEN, "flags");
static_assert(H2HP_E_PADDING == GRDMA_H2_HPACK_ERR_PADDING && H2HP_E_DEFRAMER == GRDMA_H2_HPACK_ERR_DEFRAMER, "error codes");
static_assert(sizeof(h2hp_huff_table) == sizeof(((h2hp_dev*)0)->huff) && sizeof(h2hp_static_off) == sizeof(((h2hp_dev*)0)->st_off) &&
              sizeof(h2hp_static_bytes) == sizeof(((h2hp_dev*)0)->st_bytes), "the tables as they are uploaded");

grdma_h2_hpack* grdma_h2_hpack_create(grdma_h2_parser* parser, uint32_t max_table_size, uint32_t max_block_bytes) {
  if (grdma_device_count() <= 0) return nullptr;
  if (!parser) return h2_no("h2 header decoder: no parser");
  if (parser->hpack) return h2_no("h2 header decoder: the parser has a header decoder already");
  if (max_table_size > H2HP_MAX_TABLE) return h2_no("h2 header decoder: max_table_size above 65536");
  if (max_block_bytes < 64 || max_block_bytes > (1u << 20)) return h2_no("h2 header decoder: max_block_bytes outside 64 .. 2^20");
  grdma_h2_hpack* w = new grdma_h2_hpack();
  w->parser = parser;
  w->taken = parser->standalone_calls;
  parser->hpack = w;
  bool ok = hipMalloc((void**)&w->d, sizeof(h2hp_dev)) == hipSuccess && hipMalloc((void**)&w->d_call, sizeof(h2hp_call)) == hipSuccess &&
            hipMalloc((void**)&w->d_carry, max_block_bytes) == hipSuccess && hipMemset(w->d, 0, sizeof(h2hp_dev)) == hipSuccess;
  if (ok) {
    uint8_t* d = reinterpret_cast<uint8_t*>(w->d);
    const h2hp_config cfg = {w->d_carry, max_block_bytes, max_table_size, 0};
    const uint32_t cur_max = max_table_size < 4096u ? max_table_size : 4096u;  // (RFC 7541 4.2: where the peer's encoder starts)
    ok = hipMemcpy(d + offsetof(h2hp_dev, carry_buf), &cfg, sizeof(cfg), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d + offsetof(h2hp_dev, cur_max), &cur_max, sizeof(cur_max), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d + offsetof(h2hp_dev, huff), h2hp_huff_table, sizeof(h2hp_huff_table), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d + offsetof(h2hp_dev, st_off), h2hp_static_off, sizeof(h2hp_static_off), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d + offsetof(h2hp_dev, st_bytes), h2hp_static_bytes, sizeof(h2hp_static_bytes), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    grdma_h2_hpack_destroy(w);
    grdma_fail_msg(GRDMA_ERR_HIP, "h2 header decoder: device allocation failed");
    return nullptr;
  }
  return w;
}

void grdma_h2_hpack_destroy(grdma_h2_hpack* w) {
  if (!w) return;
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);  // (standalone calls)
  if (w->parser) w->parser->hpack = nullptr;
  hipFree(w->d_blks);
  hipFree(w->d_items);
  hipFree(w->d_outs);
  hipFree(w->d_recs);
  hipFree(w->d_stage);
  hipFree(w->d_carry);
  hipFree(w->d_call);
  hipFree(w->d);
  delete w;
}

int grdma_h2_hpack_set_max_table_size(grdma_h2_hpack* w, uint32_t max_table_size) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w) return h2_invalid("h2 header decoder", "no decoder");
  if (!w->parser) return h2_invalid("h2 header decoder", "the parser is gone");
  if (max_table_size > H2HP_MAX_TABLE) return h2_invalid("h2 header decoder", "max_table_size above 65536");
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  const h2_stage stage = h2_stage_hpack_resize(w->d);
  h2_call c{"grdma_h2_hpack_set_max_table_size: a launch was rejected",
            {{reinterpret_cast<uint8_t*>(w->d) + offsetof(h2hp_dev, setting), &max_table_size, sizeof(max_table_size)}}, h2_all(stage), {}, {}};
  return h2_call_run(hc, &c);
}

// what a call of an item (the single call's arguments are one) is refused for
static const char* h2_hpack_refusal(const grdma_h2_hpack_item& it) {
  if (!it.hpack) return "a call without decoder";
  if (const char* why = h2_follow_refusal(*it.hpack, "this call is taken in already", true)) return why;
  if (!it.d_blocks || !it.blocks_cap || !it.d_fields || !it.fields_cap || !it.d_strings || !it.strings_cap || ((uintptr_t)it.d_blocks & 15) ||
      ((uintptr_t)it.d_fields & 15) || ((uintptr_t)it.d_strings & 15))
    return "a null, zero or misaligned block table, field table or string arena";
  return nullptr;
}
// where an item's call writes: the leading words of its decoder's device block
static h2hp_target h2_hpack_target(const grdma_h2_hpack_item& it) {
  return {reinterpret_cast<h2hp_block_out*>(it.d_blocks), it.blocks_cap, reinterpret_cast<h2hp_field_out*>(it.d_fields), it.fields_cap,
          static_cast<uint8_t*>(it.d_strings), it.strings_cap};
}
// the scratch words of w's device block as the host's tables stand
static h2hp_scratch h2_hpack_scratch(const grdma_h2_hpack* w) {
  return {w->d_stage, w->stage_cap, w->d_recs, w->recs_cap, w->d_outs, w->outs_cap, w->d_items, w->d_blks, std::min(w->items_cap, w->blks_cap)};
}
// in front of the gather: an item per event and the carried one; as many blocks at most
static bool h2_hpack_grow_items(grdma_h2_hpack* w) {
  const uint64_t nitems = w->parser->standalone_ev_cap + 2;
  return h2_grow(&w->d_items, &w->items_cap, nitems) && h2_grow(&w->d_blks, &w->blks_cap, nitems);
}
// what the gather of a call says: more header bytes than a call may hold (the gather commits nothing)
static bool h2_hpack_too_many(const uint64_t* pre) { return pre[0] > (1ull << 30); }
// behind the gather: the staging buffer and the record tables by the call's fragment bytes (not by the call's bytes,
// which are mostly DATA)
static bool h2_hpack_grow_scratch(grdma_h2_hpack* w, const uint64_t* pre, uint64_t fields_cap) {
  const uint64_t nouts = std::min<uint64_t>(fields_cap, pre[0]) + 1;
  return h2_grow(&w->d_stage, &w->stage_cap, pre[0] + 16) && h2_grow(&w->d_recs, &w->recs_cap, pre[0] + 1) &&
         h2_grow(&w->d_outs, &w->outs_cap, nouts);
}
// behind a call of w that ran, res its result words -> whether its blocks stand
static bool h2_hpack_ran(grdma_h2_hpack* w, float ms, const uint64_t* res) {
  // (a cap overflow, 1: nothing was written or committed, the call is not taken and may be repeated)
  h2_follow_ran(w, ms, res[H2HP_OVERFLOW] != 1);
  return res[H2HP_OVERFLOW] == 0;
}

int64_t grdma_h2_hpack_decode(grdma_h2_hpack* w, grdma_h2_header_block* d_blocks, uint64_t blocks_cap, grdma_h2_header_field* d_fields,
                              uint64_t fields_cap, void* d_strings, uint64_t strings_cap, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!out) return h2_invalid("h2 header decoder", "no result array");
  const grdma_h2_hpack_item it{w, d_blocks, blocks_cap, d_fields, fields_cap, d_strings, strings_cap};
  if (const char* why = h2_hpack_refusal(it)) return h2_invalid("h2 header decoder", why);
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  // the stream of the standalone deframings: the call is ordered behind the one it reads
  if (!h2_wait_parser(hc->stream, w->parser)) return -GRDMA_ERR_HIP;
  if (!h2_hpack_grow_items(w)) return -GRDMA_ERR_HIP;
  const h2hp_call call = h2_follow_deframed(*w);
  const h2hp_target target = h2_hpack_target(it);
  h2hp_scratch scratch = h2_hpack_scratch(w);
  uint8_t* const d = reinterpret_cast<uint8_t*>(w->d);
  uint64_t pre[4] = {0, 0, 0, 0};
  const h2_stage gather = h2_stage_hpack_gather(w->d, w->d_call);
  h2_call c1{"grdma_h2_hpack_decode: a launch was rejected",
             {{w->d_call, &call, sizeof(call)}, {d, &target, sizeof(target)}, {d + offsetof(h2hp_dev, stage), &scratch, sizeof(scratch)}}, {},
             {h2_all(gather)}, {h2_result(pre, w->d, offsetof(h2hp_dev, pre), 4)}};
  if (int rc = h2_call_run(hc, &c1)) return rc;
  if (h2_hpack_too_many(pre)) return h2_invalid("h2 header decoder", "more than 2^30 bytes of header blocks in one call");
  if (!h2_hpack_grow_scratch(w, pre, fields_cap)) return -GRDMA_ERR_HIP;
  scratch = h2_hpack_scratch(w);
  const h2_stage stage = h2_stage_hpack_decode(w->d, w->d_call);
  h2_call c2{"grdma_h2_hpack_decode: a launch was rejected", {{d + offsetof(h2hp_dev, stage), &scratch, sizeof(scratch)}}, {}, {h2_all(stage)},
             {h2_result(out, w->d, offsetof(h2hp_dev, res))}};
  if (int rc = h2_call_run(hc, &c2)) return rc;
  if (h2_hpack_ran(w, c1.ms[0] + c2.ms[0], out)) return (int64_t)out[H2HP_BLOCKS];
  if (out[H2HP_OVERFLOW] == 1)
    return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 header decoder: more blocks, fields or string bytes than the targets hold");
  return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 header decoder: the call's event list overflowed, its header blocks are lost");
}

// The decoders of many transports in the same six launches (h2_stage_hpack_links_gather, h2_stage_hpack_links_decode).
// The batch block of the process holds [table | one call block per item] (the writer batch's shape) and goes up in one
// copy; an item's targets and scratch words are the leading words of its decoder's own device block, its gather's
// figures and its result words come down from there.  Two runs, as the single call's two steps: the gathers, then --
// every decoder's scratch sized by its own figure, its scratch words sent again only where that grew something -- the other
// stages.  One call at a time, as the other batch calls.
int grdma_h2_hpack_decode_batch(const grdma_h2_hpack_item* items, uint32_t n_items, uint64_t* out) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 header decoder batch", "decoder", "h2 header decoder batch: a launch was rejected"};
  if (int rc = b.begin(items && out, n_items)) return rc;
  for (uint32_t i = 0; i < n_items; i++)
    if (int rc = b.item(items[i].hpack, h2_hpack_refusal(items[i]))) return rc;
  if (int rc = b.open(sizeof(h2hp_link), sizeof(h2hp_call), n_items)) return rc;
  auto* tab = reinterpret_cast<h2hp_link*>(b.up.data());
  auto* calls = reinterpret_cast<h2hp_call*>(b.up.data() + b.blocks);
  struct head { h2hp_target target; h2hp_scratch scratch; };  // (side by side in the device block: one copy)
  static_assert(sizeof(head) == offsetof(h2hp_dev, carry_buf) && offsetof(head, scratch) == offsetof(h2hp_dev, stage), "layout");
  std::vector<head> heads(n_items);
  std::vector<uint64_t> pre(4 * (size_t)n_items, 0);
  for (uint32_t i = 0; i < n_items; i++) {
    grdma_h2_hpack* w = items[i].hpack;
    if (!h2_hpack_grow_items(w)) return -GRDMA_ERR_HIP;
    calls[i] = h2_follow_deframed(*w);
    tab[i] = {w->d, reinterpret_cast<const h2hp_call*>(b.d + b.blocks) + i};
    heads[i] = {h2_hpack_target(items[i]), h2_hpack_scratch(w)};
    b.c.up.push_back({w->d, &heads[i], sizeof(head)});
    b.c.down.push_back(h2_result(&pre[4 * (size_t)i], w->d, offsetof(h2hp_dev, pre), 4));
    b.behind.push_back(w->parser);
  }
  const h2hp_link* d_tab = reinterpret_cast<const h2hp_link*>(b.d);
  const h2_stage gather = h2_stage_hpack_links_gather(d_tab, n_items);
  if (int rc = b.run({h2_all(gather)})) return rc;
  const float gather_ms = b.c.ms[0];
  for (uint32_t i = 0; i < n_items; i++)
    if (h2_hpack_too_many(&pre[4 * (size_t)i])) return h2_invalid(b.who, "more than 2^30 bytes of header blocks in one item's call");
  b.next();
  for (uint32_t i = 0; i < n_items; i++) {
    grdma_h2_hpack* w = items[i].hpack;
    if (!h2_hpack_grow_scratch(w, &pre[4 * (size_t)i], items[i].fields_cap)) return -GRDMA_ERR_HIP;
    const h2hp_scratch grown = h2_hpack_scratch(w);
    if (memcmp(&grown, &heads[i].scratch, sizeof(grown)) != 0) {  // (a decoder that has served such a call has room already)
      heads[i].scratch = grown;
      b.c.up.push_back({reinterpret_cast<uint8_t*>(w->d) + offsetof(h2hp_dev, stage), &heads[i].scratch, sizeof(h2hp_scratch)});
    }
    b.c.down.push_back(h2_result(out + 8 * (size_t)i, w->d, offsetof(h2hp_dev, res)));
  }
  const h2_stage stage = h2_stage_hpack_links_decode(d_tab, n_items);
  if (int rc = b.run({h2_all(stage)})) return rc;
  int ok = 0;
  for (uint32_t i = 0; i < n_items; i++)
    ok += h2_hpack_ran(items[i].hpack, gather_ms + b.c.ms[0], out + 8 * (size_t)i);  // (the time: the batch's, repeated)
  return ok;
}

int grdma_h2_hpack_table(grdma_h2_hpack* w, void* host_buf, uint64_t cap, uint64_t out[4]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w || !out || (!host_buf && cap)) return -GRDMA_ERR_INVALID;
  uint32_t st[4];  // size limit, bytes, entries, insertions
  std::vector<h2hp_entry> ring(H2HP_RING);
  std::vector<uint8_t> bytes(H2HP_BYTES);
  const uint8_t* d = reinterpret_cast<const uint8_t*>(w->d);
  if (!h2_read(st, d + offsetof(h2hp_dev, cur_max), sizeof(st)) || !h2_read(ring.data(), d + offsetof(h2hp_dev, ring), sizeof(h2hp_entry) * H2HP_RING) ||
      !h2_read(bytes.data(), d + offsetof(h2hp_dev, bytes), H2HP_BYTES))
    return -GRDMA_ERR_HIP;
  const uint32_t cnt = st[2] < H2HP_RING ? st[2] : H2HP_RING;
  uint64_t need = 0;
  for (uint32_t q = 0; q < cnt; q++) {
    const h2hp_entry& e = ring[(st[3] - 1u - q) & (H2HP_RING - 1u)];
    need += 8ull + e.name_len + e.value_len;
  }
  out[0] = cnt;
  out[1] = need;
  out[2] = st[1];
  out[3] = st[0];
  if (need > cap) return -GRDMA_ERR_CAPACITY;
  uint8_t* o = static_cast<uint8_t*>(host_buf);
  for (uint32_t q = 0; q < cnt; q++) {  // newest first: name length, value length, name, value
    const h2hp_entry& e = ring[(st[3] - 1u - q) & (H2HP_RING - 1u)];
    memcpy(o, &e.name_len, 4);
    memcpy(o + 4, &e.value_len, 4);
    o += 8;
    for (uint32_t k = 0; k < e.name_len; k++) *o++ = bytes[((e.name_src & 0x3fffffffu) + k) & (H2HP_BYTES - 1u)];
    for (uint32_t k = 0; k < e.value_len; k++) *o++ = bytes[((e.value_src & 0x3fffffffu) + k) & (H2HP_BYTES - 1u)];
  }
  return 0;
}

int grdma_h2_hpack_stats(grdma_h2_hpack* w, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w || !out) return -GRDMA_ERR_INVALID;
  uint64_t st[7];  // sticky word, then the six counters
  if (!h2_read(st, reinterpret_cast<const uint8_t*>(w->d) + offsetof(h2hp_dev, sticky), sizeof(st))) return -GRDMA_ERR_HIP;
  for (int i = 0; i < 6; i++) out[i] = st[i + 1];  // calls, blocks, fields, string bytes, inserts, evictions
  out[6] = st[0];
  out[7] = (uint64_t)(w->last_ms * 1e6f);
  return 0;
}

// ---- header blocks, sending: the HPACK encoder on the device (csrc/grdma_h2_hpenc.h) ----------------------------------------
// The encoder follows no parser: its input is three device tables of the caller.  The peer's settings live on the host
// until a call that sends a block takes them in (a refused call leaves them pending); a call is one run of the stage,
// repeated once where the occurrence table was too small (blocks may share fields: only the device can count them).
struct grdma_h2_hpenc {
  h2he_dev* d = nullptr;
  h2he_rec* d_recs = nullptr;
  uint64_t recs_cap = 0;
  h2he_occ* d_occs = nullptr;
  uint64_t occs_cap = 0;
  h2he_blk* d_blks = nullptr;
  uint64_t blks_cap = 0;
  uint32_t cur = 0, want = 0, low = 0;  // the limit the peer's decoder is at; what the peer asked for; the lowest since the last block
  uint32_t max_frame = 0;
  float ms[3] = {0, 0, 0};  // of the last call: scan, walk, emit and commit
};
static_assert(sizeof(h2he_wire_out) == sizeof(grdma_h2_header_wire) && H2HE_F_BAD_INPUT == GRDMA_H2_HPENC_BAD_INPUT &&
              H2HE_E_FIELD_RANGE == GRDMA_H2_HPENC_ERR_FIELD_RANGE && H2HE_E_BLOCK_TOO_LARGE == GRDMA_H2_HPENC_ERR_BLOCK_TOO_LARGE, "layout");
static_assert(offsetof(h2he_dev, c) == 0 && sizeof(h2he_huff_code) == sizeof(((h2he_dev*)0)->huff_code) &&
              sizeof(h2he_huff_bits) == sizeof(((h2he_dev*)0)->huff_bits) && sizeof(h2he_static_name_hash) == sizeof(((h2he_dev*)0)->st_hn) &&
              sizeof(h2he_static_full_hash) == sizeof(((h2he_dev*)0)->st_hf) && sizeof(h2hp_static_off) == sizeof(((h2he_dev*)0)->st_off) &&
              sizeof(h2hp_static_bytes) == sizeof(((h2he_dev*)0)->st_bytes), "the call's words lead the block; the tables as they are uploaded");

static const char* h2_hpenc_bad_peer(uint32_t peer_table_size, uint32_t peer_max_frame) {
  if (peer_table_size > H2HP_MAX_TABLE) return "peer_table_size above 65536";
  if (peer_max_frame < 16384u || peer_max_frame > 0xffffffu) return "peer_max_frame outside 16384 .. 2^24 - 1";
  return nullptr;
}

grdma_h2_hpenc* grdma_h2_hpenc_create(uint32_t peer_table_size, uint32_t peer_max_frame) {
  if (grdma_device_count() <= 0) return nullptr;
  if (const char* why = h2_hpenc_bad_peer(peer_table_size, peer_max_frame)) {
    h2_invalid("h2 header encoder", why);
    return nullptr;
  }
  grdma_h2_hpenc* w = new grdma_h2_hpenc();
  // (RFC 7541 4.2: both sides begin at 4096 or at the peer's setting where that is less; more is announced in the first block)
  w->cur = w->low = peer_table_size < 4096u ? peer_table_size : 4096u;
  w->want = peer_table_size;
  w->max_frame = peer_max_frame;
  bool ok = hipMalloc((void**)&w->d, sizeof(h2he_dev)) == hipSuccess && hipMemset(w->d, 0, sizeof(h2he_dev)) == hipSuccess;
  if (ok) {
    uint8_t* d = reinterpret_cast<uint8_t*>(w->d);
    ok = hipMemcpy(d + offsetof(h2he_dev, cur_max), &w->cur, sizeof(w->cur), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d + offsetof(h2he_dev, huff_code), h2he_huff_code, sizeof(h2he_huff_code), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d + offsetof(h2he_dev, huff_bits), h2he_huff_bits, sizeof(h2he_huff_bits), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d + offsetof(h2he_dev, st_hn), h2he_static_name_hash, sizeof(h2he_static_name_hash), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d + offsetof(h2he_dev, st_hf), h2he_static_full_hash, sizeof(h2he_static_full_hash), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d + offsetof(h2he_dev, st_off), h2hp_static_off, sizeof(h2hp_static_off), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d + offsetof(h2he_dev, st_bytes), h2hp_static_bytes, sizeof(h2hp_static_bytes), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    grdma_h2_hpenc_destroy(w);
    grdma_fail_msg(GRDMA_ERR_HIP, "h2 header encoder: device allocation failed");
    return nullptr;
  }
  return w;
}

void grdma_h2_hpenc_destroy(grdma_h2_hpenc* w) {
  if (!w) return;
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);  // (standalone calls)
  hipFree(w->d_blks);
  hipFree(w->d_occs);
  hipFree(w->d_recs);
  hipFree(w->d);
  delete w;
}

int grdma_h2_hpenc_set_peer(grdma_h2_hpenc* w, uint32_t peer_table_size, uint32_t peer_max_frame) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w) return h2_invalid("h2 header encoder", "no encoder");
  if (const char* why = h2_hpenc_bad_peer(peer_table_size, peer_max_frame)) return h2_invalid("h2 header encoder", why);
  w->want = peer_table_size;
  w->low = std::min(w->low, peer_table_size);
  w->max_frame = peer_max_frame;
  return 0;
}

// what a call of an item (the single call's arguments are one) is refused for
static const char* h2_hpenc_refusal(const grdma_h2_hpenc_item& it) {
  if (!it.enc) return "no encoder";
  if (!it.d_wire || !it.wire_cap || !it.d_block_wire || !it.block_wire_cap || ((uintptr_t)it.d_wire & 15) || ((uintptr_t)it.d_block_wire & 15))
    return "a null, zero or misaligned wire arena or block-wire table";
  if ((it.nblocks && !it.d_blocks) || (it.nfields && !it.d_fields) || (it.strings_bytes && !it.d_strings) || ((uintptr_t)it.d_blocks & 15) ||
      ((uintptr_t)it.d_fields & 15))
    return "a null or misaligned block table, field table or string arena";
  if (it.nblocks >= 0xffffffffull || it.nfields > 0xffffffffull || it.strings_bytes > (1ull << 32))
    return "more than 2^32 - 1 blocks or fields, or a string arena above 2^32 bytes";
  return nullptr;
}
// in front of a call: a record per field, a row per block and one behind, an occurrence per field and some (blocks that
// share fields hold more: only the device can count them)
static bool h2_hpenc_grow(const grdma_h2_hpenc_item& it) {
  grdma_h2_hpenc* w = it.enc;
  return h2_grow(&w->d_recs, &w->recs_cap, it.nfields + 1) && h2_grow(&w->d_blks, &w->blks_cap, it.nblocks + 2) &&
         h2_grow(&w->d_occs, &w->occs_cap, it.nfields + 64);
}
// the call's words as the encoder's tables and the peer's pending settings stand
static h2he_call h2_hpenc_call(const grdma_h2_hpenc_item& it) {
  const grdma_h2_hpenc* w = it.enc;
  h2he_call call = {reinterpret_cast<const h2hp_block_out*>(it.d_blocks), it.nblocks, reinterpret_cast<const h2hp_field_out*>(it.d_fields), it.nfields,
                    static_cast<const uint8_t*>(it.d_strings), it.strings_bytes, static_cast<uint8_t*>(it.d_wire), it.wire_cap,
                    reinterpret_cast<h2he_wire_out*>(it.d_block_wire), it.block_wire_cap, w->d_recs, w->recs_cap, w->d_occs, w->occs_cap,
                    w->d_blks, w->blks_cap, w->max_frame, 0, {0, 0}};
  if (w->low < w->want && w->low < w->cur) {  // lowered, then raised: the smallest since the last block, then the final one (4.2)
    call.nupd = 2;
    call.upd[0] = w->low;
    call.upd[1] = w->want;
  } else if (w->want != w->cur) {
    call.nupd = 1;
    call.upd[0] = w->want;
  }
  return call;
}
// down: a run's nine words (the result block, the occurrence count).  Whether the run said the occurrence table is too
// small: then the table is grown for one more run (*rc 0), or the call is refused (*rc: what it returns)
static bool h2_hpenc_again(grdma_h2_hpenc* w, const char* who, const uint64_t* down, int attempt, int* rc) {
  if (down[H2HE_OVERFLOW] != H2HE_OVER_SCRATCH) return false;
  if (attempt || down[8] >= 0xffffffffull) *rc = h2_invalid(who, "more than 2^32 - 1 fields in the call's blocks");
  else *rc = h2_grow(&w->d_occs, &w->occs_cap, down[8] + 64) ? 0 : -GRDMA_ERR_HIP;
  return true;
}
// behind a call of an item that ran, res its result words, ms the call's three sections -> whether its blocks are on the wire
static bool h2_hpenc_ran(const grdma_h2_hpenc_item& it, const uint64_t* res, const float* ms) {
  grdma_h2_hpenc* w = it.enc;
  for (int k = 0; k < 3; k++) w->ms[k] = ms[k];
  if ((res[H2HE_FLAGS] & H2HE_F_BAD_INPUT) || res[H2HE_OVERFLOW]) return false;
  if (it.nblocks) w->cur = w->low = w->want;  // (the block that said so is out)
  return true;
}

int64_t grdma_h2_hpenc_encode(grdma_h2_hpenc* w, const grdma_h2_header_block* d_blocks, uint64_t nblocks, const grdma_h2_header_field* d_fields,
                              uint64_t nfields, const void* d_strings, uint64_t strings_bytes, void* d_wire, uint64_t wire_cap,
                              grdma_h2_header_wire* d_block_wire, uint64_t block_wire_cap, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  const char* who = "h2 header encoder";
  const grdma_h2_hpenc_item it{w, d_blocks, nblocks, d_fields, nfields, d_strings, strings_bytes, d_wire, wire_cap, d_block_wire, block_wire_cap};
  if (w && !out) return h2_invalid(who, "no result array");
  if (const char* why = h2_hpenc_refusal(it)) return h2_invalid(who, why);
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  if (!h2_hpenc_grow(it)) return -GRDMA_ERR_HIP;
  uint64_t down[9];  // the result block and the occurrence count behind it
  static_assert(offsetof(h2he_dev, nocc) == offsetof(h2he_dev, res) + 8 * sizeof(uint64_t), "one download");
  float ms[3] = {0, 0, 0};
  const h2_stage stage = h2_stage_hpenc(w->d);
  for (int attempt = 0;; attempt++) {
    const h2he_call call = h2_hpenc_call(it);
    h2_call c{"grdma_h2_hpenc_encode: a launch was rejected", {{w->d, &call, sizeof(call)}}, {},
              {{stage.data(), 1}, {stage.data() + 1, 1}, {stage.data() + 2, 2}}, {h2_result(down, w->d, offsetof(h2he_dev, res), 9)}};
    if (int rc = h2_call_run(hc, &c)) return rc;
    for (int k = 0; k < 3; k++) w->ms[k] = ms[k] = c.ms[k];
    int rc = 0;
    if (!h2_hpenc_again(w, who, down, attempt, &rc)) break;
    if (rc) return rc;
  }
  for (int k = 0; k < 8; k++) out[k] = down[k];
  if (h2_hpenc_ran(it, down, ms)) return (int64_t)out[H2HE_FRAMES];
  if (out[H2HE_FLAGS] & H2HE_F_BAD_INPUT) return h2_invalid(who, "bad input: a block's fields, a string, a stream id or a length (the result block says which block)");
  return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 header encoder: more wire bytes or blocks than the targets hold");
}

// The encoders of many connections in the same four launches (h2_stage_hpenc_links).  The batch block of the process
// holds [table | one h2he_call per item | nine result words per item]: the table and the call words go up in ONE copy,
// the result words come down in ONE copy, whatever the number of items -- nothing of a call passes through the encoders'
// own device blocks, whose words stay the single call's.  Items whose occurrence table was too small (blocks that share
// fields) get it grown and run once more, in a second run of the four launches over a table of those items only: the
// walk commits, so an item that stood in the first run is never run twice.  One call at a time, as the other batch calls.
int grdma_h2_hpenc_encode_batch(const grdma_h2_hpenc_item* items, uint32_t n_items, uint64_t* out) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 header encoder batch", "encoder", "h2 header encoder batch: a launch was rejected"};
  if (int rc = b.begin(items && out, n_items)) return rc;
  for (uint32_t i = 0; i < n_items; i++)
    if (int rc = b.item(items[i].enc, h2_hpenc_refusal(items[i]))) return rc;
  for (uint32_t i = 0; i < n_items; i++)
    if (!h2_hpenc_grow(items[i])) return -GRDMA_ERR_HIP;
  std::vector<uint32_t> todo(n_items);  // the items of the run
  for (uint32_t i = 0; i < n_items; i++) todo[i] = i;
  std::vector<uint64_t> res(9 * (size_t)n_items, 0), down;
  float ms[3] = {0, 0, 0};
  int refused = 0;  // what the call returns for an item whose occurrence table cannot be made to hold its blocks
  for (int attempt = 0; !todo.empty(); attempt++) {
    const uint32_t n = (uint32_t)todo.size();
    const h2_hpenc_block L = h2_hpenc_block_layout(sizeof(h2he_link), sizeof(h2he_call), n);
    if (attempt) b.next();
    if (int rc = b.reserve(L.results, L.total)) return rc;
    auto* tab = reinterpret_cast<h2he_link*>(b.up.data() + L.tab);
    auto* calls = reinterpret_cast<h2he_call*>(b.up.data() + L.calls);
    for (uint32_t k = 0; k < n; k++) {
      calls[k] = h2_hpenc_call(items[todo[k]]);
      tab[k] = {items[todo[k]].enc->d, reinterpret_cast<const h2he_call*>(b.d + L.calls) + k, reinterpret_cast<uint64_t*>(b.d + L.results) + 9 * (size_t)k};
    }
    down.assign(9 * (size_t)n, 0);
    b.c.down.push_back(h2_result(down.data(), b.d, L.results, 9 * (size_t)n));
    const h2_stage stage = h2_stage_hpenc_links(reinterpret_cast<const h2he_link*>(b.d + L.tab), n);
    if (int rc = b.run({{stage.data(), 1}, {stage.data() + 1, 1}, {stage.data() + 2, 2}})) return rc;
    for (int k = 0; k < 3; k++) ms[k] += b.c.ms[k];
    std::vector<uint32_t> again;
    for (uint32_t k = 0; k < n; k++) {
      const uint32_t i = todo[k];
      memcpy(&res[9 * (size_t)i], &down[9 * (size_t)k], 9 * sizeof(uint64_t));
      int rc = 0;
      if (!h2_hpenc_again(items[i].enc, b.who, &down[9 * (size_t)k], attempt, &rc)) continue;
      if (rc && !refused) refused = rc;
      again.push_back(i);
    }
    todo.swap(again);
    if (refused) break;
  }
  // (after a refusal the items that stood stay committed on the device: the host takes their results in all the same)
  int ok = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    if (res[9 * (size_t)i + H2HE_OVERFLOW] == H2HE_OVER_SCRATCH) continue;
    memcpy(out + 8 * (size_t)i, &res[9 * (size_t)i], 8 * sizeof(uint64_t));
    ok += h2_hpenc_ran(items[i], &res[9 * (size_t)i], ms);  // (the times: the batch's, repeated)
  }
  return todo.empty() ? ok : refused;
}


int grdma_h2_hpenc_table(grdma_h2_hpenc* w, void* host_buf, uint64_t cap, uint64_t out[4]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w || !out || (!host_buf && cap)) return -GRDMA_ERR_INVALID;
  uint32_t st[4];  // size limit, bytes, entries, insertions
  std::vector<uint32_t> nl(H2HP_RING), vl(H2HP_RING), src(H2HP_RING);
  std::vector<uint8_t> bytes(H2HP_BYTES);
  const uint8_t* d = reinterpret_cast<const uint8_t*>(w->d);
  if (!h2_read(st, d + offsetof(h2he_dev, cur_max), sizeof(st)) || !h2_read(nl.data(), d + offsetof(h2he_dev, r_nl), 4 * H2HP_RING) ||
      !h2_read(vl.data(), d + offsetof(h2he_dev, r_vl), 4 * H2HP_RING) || !h2_read(src.data(), d + offsetof(h2he_dev, r_src), 4 * H2HP_RING) ||
      !h2_read(bytes.data(), d + offsetof(h2he_dev, bytes), H2HP_BYTES))
    return -GRDMA_ERR_HIP;
  const uint32_t cnt = st[2] < H2HP_RING ? st[2] : H2HP_RING;
  uint64_t need = 0;
  for (uint32_t q = 0; q < cnt; q++) {
    const uint32_t slot = (st[3] - 1u - q) & (H2HP_RING - 1u);
    need += 8ull + nl[slot] + vl[slot];
  }
  out[0] = cnt;
  out[1] = need;
  out[2] = st[1];
  out[3] = st[0];
  if (need > cap) return -GRDMA_ERR_CAPACITY;
  uint8_t* o = static_cast<uint8_t*>(host_buf);
  for (uint32_t q = 0; q < cnt; q++) {  // newest first: name length, value length, name, value (grdma_h2_hpack_table's format)
    const uint32_t slot = (st[3] - 1u - q) & (H2HP_RING - 1u);
    memcpy(o, &nl[slot], 4);
    memcpy(o + 4, &vl[slot], 4);
    o += 8;
    for (uint32_t k = 0; k < nl[slot] + vl[slot]; k++) *o++ = bytes[(src[slot] + k) & (H2HP_BYTES - 1u)];
  }
  return 0;
}

int grdma_h2_hpenc_stats(grdma_h2_hpenc* w, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w || !out) return -GRDMA_ERR_INVALID;
  // calls, blocks, fields, header-list bytes in, wire bytes out, inserts, evictions
  if (!h2_read(out, reinterpret_cast<const uint8_t*>(w->d) + offsetof(h2he_dev, st_calls), 7 * sizeof(uint64_t))) return -GRDMA_ERR_HIP;
  out[7] = (uint64_t)((w->ms[0] + w->ms[1] + w->ms[2]) * 1e6f);
  return 0;
}

int grdma_h2_hpenc_last_stages(grdma_h2_hpenc* w, uint64_t out[4]) {
  if (!w || !out) return -GRDMA_ERR_INVALID;
  for (int k = 0; k < 3; k++) out[k] = (uint64_t)(w->ms[k] * 1e6f);
  out[3] = out[0] + out[1] + out[2];
  return 0;
}

// ---- call metadata: the metadata reader on the device (csrc/grdma_h2_meta.h) ------------------------------------------------
// The reader follows no parser: its input is three device tables of the caller.  What it owns in device memory is
// constant after creation -- the method table, the known keys, the field table and the string arena of the rejection
// lists -- and a call is one run of the stage.
struct grdma_h2_meta {
  h2m_dev* d = nullptr;
  h2m_slot* d_slots = nullptr;
  uint8_t* d_paths = nullptr;
  grdma_h2_header_field* d_rej_fields = nullptr;
  uint8_t* d_rej_strings = nullptr;
  uint64_t rej_nfields = 0, rej_bytes = 0;
  h2m_rec* d_recs = nullptr;
  uint64_t recs_cap = 0;
  h2m_meta_out* d_mrecs = nullptr;
  uint64_t mrecs_cap = 0;
  float ms = 0;  // of the last call
};
static_assert(sizeof(h2m_meta_out) == sizeof(grdma_h2_call_meta) && sizeof(grdma_h2_call_meta) == 48 && offsetof(h2m_dev, c) == 0 &&
              H2M_F_BAD_INPUT == GRDMA_H2_META_BAD_INPUT && H2M_E_STRING == GRDMA_H2_META_ERR_STRING &&
              H2M_IS_TRAILERS == GRDMA_H2_META_TRAILERS && H2M_BAD_GRPC_STATUS == GRDMA_H2_META_BAD_GRPC_STATUS &&
              H2M_HAS_MESSAGE == GRDMA_H2_META_HAS_MESSAGE && sizeof(h2m_key_off) <= sizeof(((h2m_dev*)0)->key_off) &&
              sizeof(h2m_key_bytes) <= sizeof(((h2m_dev*)0)->key_bytes), "layout");

grdma_h2_meta* grdma_h2_meta_create(const void* methods, uint64_t methods_bytes, uint32_t nmethods, uint32_t accept_encodings) {
  if (grdma_device_count() <= 0) return nullptr;
  if (nmethods > 4096u) return h2_no("h2 metadata reader: more than 4096 methods");
  if ((accept_encodings >> 3) || !(accept_encodings & 1u)) return h2_no("h2 metadata reader: accept_encodings has bits above 7 or lacks identity");
  if (!methods && (nmethods || methods_bytes)) return h2_no("h2 metadata reader: no method list");
  // the method table: open addressing over a power of two >= 2 n slots, FNV-1a, linear probing
  uint32_t nslots = 2;
  while (nslots < 2u * nmethods) nslots *= 2;
  std::vector<h2m_slot> slots(nslots, h2m_slot{0, 0, 0, 0});
  std::vector<uint8_t> paths;
  const uint8_t* p = static_cast<const uint8_t*>(methods);
  uint64_t pos = 0;
  for (uint32_t i = 0; i < nmethods; i++) {
    uint32_t len = 0;
    if (pos + 4 > methods_bytes) return h2_no("h2 metadata reader: the method list ends inside an entry");
    memcpy(&len, p + pos, 4);
    pos += 4;
    if (len < 1u || len > 1024u) return h2_no("h2 metadata reader: a path outside 1 .. 1024 bytes");
    if (pos + len > methods_bytes) return h2_no("h2 metadata reader: the method list ends inside an entry");
    uint32_t h = 0x811c9dc5u;
    for (uint32_t k = 0; k < len; k++) h = (h ^ p[pos + k]) * 0x01000193u;
    uint32_t at = h & (nslots - 1u);
    for (; slots[at].len; at = (at + 1u) & (nslots - 1u))
      if (slots[at].hash == h && slots[at].len == len && !memcmp(paths.data() + slots[at].off, p + pos, len))
        return h2_no("h2 metadata reader: a path twice");
    slots[at] = h2m_slot{h, (uint32_t)paths.size(), len, i};
    paths.insert(paths.end(), p + pos, p + pos + len);
    pos += len;
  }
  if (pos != methods_bytes) return h2_no("h2 metadata reader: the method list does not end at methods_bytes");
  // the rejection lists (rule 8): per verdict :status, content-type, grpc-status, grpc-message, all with hint 1
  std::vector<grdma_h2_header_field> rf;
  std::vector<uint8_t> rs;
  std::vector<uint8_t> mirror(sizeof(h2m_dev), 0);
  h2m_dev* m = reinterpret_cast<h2m_dev*>(mirror.data());
  auto put = [&](const char* name, const std::string& value) {
    const uint32_t nl = (uint32_t)strlen(name), off = (uint32_t)rs.size();
    rf.push_back(grdma_h2_header_field{off, off + nl, nl | 1u << 24, (uint32_t)value.size()});
    rs.insert(rs.end(), name, name + nl);
    rs.insert(rs.end(), value.begin(), value.end());
  };
  for (const h2m_rejection& r : h2m_rejections) {
    m->rej_first[r.verdict] = (uint32_t)rf.size();
    put(":status", r.status);
    put("content-type", H2M_CONTENT_TYPE);
    put("grpc-status", r.grpc_status);
    put("grpc-message", r.message);
    if (r.verdict == H2M_BAD_ENCODING) {
      std::string set;
      for (uint32_t k = 0; k < 3; k++)
        if ((accept_encodings >> k) & 1u) set += (set.empty() ? "" : ",") + std::string(h2m_encodings[k]);
      put("grpc-accept-encoding", set);
    }
    m->rej_n[r.verdict] = (uint32_t)rf.size() - m->rej_first[r.verdict];
  }
  grdma_h2_meta* w = new grdma_h2_meta();
  w->rej_nfields = rf.size();
  w->rej_bytes = rs.size();
  bool ok = hipMalloc((void**)&w->d, sizeof(h2m_dev)) == hipSuccess && hipMalloc((void**)&w->d_slots, sizeof(h2m_slot) * nslots) == hipSuccess &&
            hipMalloc((void**)&w->d_paths, paths.size() + 16) == hipSuccess &&
            hipMalloc((void**)&w->d_rej_fields, sizeof(grdma_h2_header_field) * rf.size()) == hipSuccess &&
            hipMalloc((void**)&w->d_rej_strings, rs.size() + 16) == hipSuccess;
  if (ok) {
    m->slots = w->d_slots;
    m->paths = w->d_paths;
    m->slot_mask = nslots - 1u;
    m->accept = accept_encodings;
    memcpy(m->key_off, h2m_key_off, sizeof(h2m_key_off));
    memcpy(m->key_bytes, h2m_key_bytes, sizeof(h2m_key_bytes));
    for (h2m_wg& g : m->wg) g.bad = ~0ull;
    ok = hipMemcpy(w->d, m, sizeof(h2m_dev), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(w->d_slots, slots.data(), sizeof(h2m_slot) * nslots, hipMemcpyHostToDevice) == hipSuccess &&
         (paths.empty() || hipMemcpy(w->d_paths, paths.data(), paths.size(), hipMemcpyHostToDevice) == hipSuccess) &&
         hipMemcpy(w->d_rej_fields, rf.data(), sizeof(grdma_h2_header_field) * rf.size(), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(w->d_rej_strings, rs.data(), rs.size(), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    grdma_h2_meta_destroy(w);
    grdma_fail_msg(GRDMA_ERR_HIP, "h2 metadata reader: device allocation failed");
    return nullptr;
  }
  return w;
}

void grdma_h2_meta_destroy(grdma_h2_meta* w) {
  if (!w) return;
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);  // (standalone calls; an encode of the rejection lists reads the constant tables)
  hipFree(w->d_mrecs);
  hipFree(w->d_recs);
  hipFree(w->d_rej_strings);
  hipFree(w->d_rej_fields);
  hipFree(w->d_paths);
  hipFree(w->d_slots);
  hipFree(w->d);
  delete w;
}

// what a call of an item (the single call's arguments are one) is refused for
static const char* h2_meta_refusal(const grdma_h2_meta_item& it) {
  if (!it.d_meta || !it.meta_cap || !it.d_reject || !it.reject_cap || ((uintptr_t)it.d_meta & 15) || ((uintptr_t)it.d_reject & 15))
    return "a null, zero or misaligned record table or rejection list";
  if ((it.nblocks && !it.d_blocks) || (it.nfields && !it.d_fields) || (it.strings_bytes && !it.d_strings) || ((uintptr_t)it.d_blocks & 15) ||
      ((uintptr_t)it.d_fields & 15))
    return "a null or misaligned block table, field table or string arena";
  if (it.nblocks >= 0xffffffffull || it.nfields > 0xffffffffull || it.strings_bytes > (1ull << 32))
    return "more than 2^32 - 1 blocks or fields, or a string arena above 2^32 bytes";
  return nullptr;
}
// the call's words of an item over its part of the reader's scratch: a record per field, a call record per block
static h2m_call h2_meta_call(const grdma_h2_meta_item& it, h2m_rec* recs, uint64_t recs_cap, h2m_meta_out* mrecs, uint64_t mrecs_cap) {
  return {reinterpret_cast<const h2hp_block_out*>(it.d_blocks), it.nblocks, reinterpret_cast<const h2hp_field_out*>(it.d_fields), it.nfields,
          static_cast<const uint8_t*>(it.d_strings), it.strings_bytes, reinterpret_cast<h2m_meta_out*>(it.d_meta), it.meta_cap,
          reinterpret_cast<h2hp_block_out*>(it.d_reject), it.reject_cap, recs, recs_cap, mrecs, mrecs_cap};
}
// whether an item's result words say it was read
static bool h2_meta_was_read(const uint64_t* res) { return !(res[H2M_FLAGS] & H2M_F_BAD_INPUT) && !res[H2M_OVERFLOW]; }

int64_t grdma_h2_meta_read(grdma_h2_meta* w, const grdma_h2_header_block* d_blocks, uint64_t nblocks, const grdma_h2_header_field* d_fields,
                           uint64_t nfields, const void* d_strings, uint64_t strings_bytes, grdma_h2_call_meta* d_meta, uint64_t meta_cap,
                           grdma_h2_header_block* d_reject, uint64_t reject_cap, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  const char* who = "h2 metadata reader";
  if (!w) return h2_invalid(who, "no reader");
  if (!out) return h2_invalid(who, "no result array");
  const grdma_h2_meta_item it{d_blocks, nblocks, d_fields, nfields, d_strings, strings_bytes, d_meta, meta_cap, d_reject, reject_cap};
  if (const char* why = h2_meta_refusal(it)) return h2_invalid(who, why);
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  if (!h2_grow(&w->d_recs, &w->recs_cap, nfields + 1) || !h2_grow(&w->d_mrecs, &w->mrecs_cap, nblocks + 1)) return -GRDMA_ERR_HIP;
  const h2m_call call = h2_meta_call(it, w->d_recs, w->recs_cap, w->d_mrecs, w->mrecs_cap);
  const h2_stage stage = h2_stage_meta(w->d);
  h2_call c{"grdma_h2_meta_read: a launch was rejected", {{w->d, &call, sizeof(call)}}, {}, {h2_all(stage)},
            {h2_result(out, w->d, offsetof(h2m_dev, res))}};
  if (int rc = h2_call_run(hc, &c)) return rc;
  w->ms = c.ms[0];
  if (out[H2M_FLAGS] & H2M_F_BAD_INPUT) return h2_invalid(who, "bad input: a block's fields, a stream id or a string (the result block says which block)");
  if (out[H2M_OVERFLOW]) return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 metadata reader: more blocks or rejections than the targets hold");
  return (int64_t)out[H2M_REJECTIONS];
}

// n items through the ONE reader in the same three launches (h2_stage_meta_links).  The batch block of the process holds
// [table | one h2m_call per item | the items' workgroup counts | eight result words per item] (csrc/grdma_h2_block.h):
// the table, the call words and the counts' fill go up in ONE copy, the result words come down in ONE copy, whatever
// the number of items -- nothing of a call passes through the reader's own device block but the counters, which the
// emit launch bumps once.  An item's records and call records are its slice of the reader's scratch, grown to the sum
// over the items and one more each (a slice starts on 16 bytes: both records are multiples of 16 bytes long).  One
// call at a time, as the other batch calls.
int grdma_h2_meta_read_batch(grdma_h2_meta* w, const grdma_h2_meta_item* items, uint32_t n_items, uint64_t* out) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 metadata reader batch", "item", "grdma_h2_meta_read_batch: a launch was rejected"};
  if (!w) return h2_invalid(b.who, "no reader");
  if (!items) return h2_invalid(b.who, "no item array");
  if (!out) return h2_invalid(b.who, "no result array");
  if (int rc = b.begin(true, n_items)) return rc;
  uint64_t nrecs = 0, nmrecs = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    if (int rc = b.item(nullptr, h2_meta_refusal(items[i]))) return rc;
    nrecs += items[i].nfields + 1;
    nmrecs += items[i].nblocks + 1;
  }
  static_assert(sizeof(h2m_rec) % 16 == 0 && sizeof(h2m_meta_out) % 16 == 0, "a slice of the scratch starts on 16 bytes");
  const h2_meta_block L = h2_meta_block_layout(sizeof(h2m_link), sizeof(h2m_call), sizeof(h2m_wg), H2M_LINK_GRID, n_items);
  if (int rc = b.reserve(L.results, L.total)) return rc;
  if (!h2_grow(&w->d_recs, &w->recs_cap, nrecs) || !h2_grow(&w->d_mrecs, &w->mrecs_cap, nmrecs)) return -GRDMA_ERR_HIP;
  auto* tab = reinterpret_cast<h2m_link*>(b.up.data() + L.tab);
  auto* calls = reinterpret_cast<h2m_call*>(b.up.data() + L.calls);
  auto* wgs = reinterpret_cast<h2m_wg*>(b.up.data() + L.wgs);
  uint64_t rec0 = 0, mrec0 = 0;
  for (uint32_t i = 0; i < n_items; i++) {
    calls[i] = h2_meta_call(items[i], w->d_recs + rec0, items[i].nfields + 1, w->d_mrecs + mrec0, items[i].nblocks + 1);
    rec0 += items[i].nfields + 1;
    mrec0 += items[i].nblocks + 1;
    for (uint32_t k = 0; k < H2M_LINK_GRID; k++) wgs[(size_t)i * H2M_LINK_GRID + k].bad = ~0ull;
    tab[i] = {reinterpret_cast<const h2m_call*>(b.d + L.calls) + i, reinterpret_cast<h2m_wg*>(b.d + L.wgs) + (size_t)i * H2M_LINK_GRID,
              reinterpret_cast<uint64_t*>(b.d + L.results) + 8 * (size_t)i};
  }
  std::vector<uint64_t> down(8 * (size_t)n_items, 0);  // (out is not touched unless the call ran)
  b.c.down.push_back(h2_result(down.data(), b.d, L.results, down.size()));
  const h2_stage stage = h2_stage_meta_links(w->d, reinterpret_cast<const h2m_link*>(b.d + L.tab), n_items);
  if (int rc = b.run({h2_all(stage)})) return rc;
  w->ms = b.c.ms[0];
  memcpy(out, down.data(), down.size() * sizeof(uint64_t));
  int read = 0;
  for (uint32_t i = 0; i < n_items; i++) read += h2_meta_was_read(out + 8 * (size_t)i);
  return read;
}

int grdma_h2_meta_reject_tables(grdma_h2_meta* w, uint64_t out[4]) {
  if (!w || !out) return -GRDMA_ERR_INVALID;
  out[0] = (uint64_t)(uintptr_t)w->d_rej_fields;
  out[1] = w->rej_nfields;
  out[2] = (uint64_t)(uintptr_t)w->d_rej_strings;
  out[3] = w->rej_bytes;
  return 0;
}

int grdma_h2_meta_stats(grdma_h2_meta* w, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w || !out) return -GRDMA_ERR_INVALID;
  // calls, blocks, requests, responses, trailers, rejections, malformed
  if (!h2_read(out, reinterpret_cast<const uint8_t*>(w->d) + offsetof(h2m_dev, st_calls), 7 * sizeof(uint64_t))) return -GRDMA_ERR_HIP;
  out[7] = (uint64_t)(w->ms * 1e6f);
  return 0;
}

// ---- the call table (csrc/grdma_h2_calls.h) -----------------------------------------------------------------------------------
// The table follows no parser: a step's input is four device tables of the caller.  What it owns in device memory is the
// two entry tables, the count rows (sized at creation) and the scratch that grows with a step's records and descriptors.
struct grdma_h2_calls {
  h2c_dev* d = nullptr;
  h2c_dev h;  // the words set at creation
  uint32_t* d_cls = nullptr;
  uint64_t cls_cap = 0;
  h2c_dd* d_dd = nullptr;
  uint64_t dd_cap = 0;
  h2c_mrec* d_mrec = nullptr;
  uint64_t mrec_cap = 0;
  float ms = 0;  // of the last step
};
static_assert(sizeof(h2c_disp) == sizeof(grdma_h2_dispatch) && sizeof(grdma_h2_dispatch) == 48 && sizeof(h2c_done) == sizeof(grdma_h2_call_done) &&
              sizeof(grdma_h2_call_done) == 32 && sizeof(h2c_entry) == sizeof(grdma_h2_call_entry) && sizeof(grdma_h2_call_entry) == 48 &&
              sizeof(h2c_msg) == sizeof(grdma_h2_rx_msg) && offsetof(h2c_dev, c) == 0 && H2C_F_BAD_INPUT == GRDMA_H2_CALLS_BAD_INPUT &&
              H2C_F_LOST == GRDMA_H2_CALLS_LOST && H2C_E_METHOD == GRDMA_H2_CALLS_ERR_METHOD && H2C_COMPRESSED_IDENTITY == GRDMA_H2_ORPHAN_COMPRESSED_IDENTITY &&
              H2C_DEADLINE == GRDMA_H2_DONE_DEADLINE && H2C_COMPRESSED == GRDMA_H2_DISPATCH_COMPRESSED, "layout");

void grdma_h2_calls_destroy(grdma_h2_calls* w) {
  if (!w) return;
  h2_host_ctx* hc = h2_ctx();
  if (hc) hipStreamSynchronize(hc->stream);
  hipFree(w->d_mrec);
  hipFree(w->d_dd);
  hipFree(w->d_cls);
  hipFree(w->h.exp_rank);
  hipFree(w->h.exp_slot);
  hipFree(w->h.ktot);
  hipFree(w->h.row_k);
  hipFree(w->h.row_s);
  hipFree(w->h.aux);
  hipFree(w->h.tab[1]);
  hipFree(w->h.tab[0]);
  hipFree(w->d);
  delete w;
}

grdma_h2_calls* grdma_h2_calls_create(uint32_t table_slots, uint32_t nmethods) {
  if (grdma_device_count() <= 0) return nullptr;
  if (!table_slots) table_slots = 4096;
  if (table_slots < 16u || table_slots > H2C_SLOTS_MAX || (table_slots & (table_slots - 1u)))
    return h2_no("h2 call table: table_slots is no power of two in 16 .. 65536");
  if (nmethods > 4096u) return h2_no("h2 call table: more than 4096 methods");
  grdma_h2_calls* w = new grdma_h2_calls();
  memset(&w->h, 0, sizeof(w->h));
  h2c_dev* m = &w->h;
  const size_t slots = table_slots;
  bool ok = hipMalloc((void**)&w->d, sizeof(h2c_dev)) == hipSuccess && hipMalloc((void**)&m->tab[0], sizeof(h2c_entry) * slots) == hipSuccess &&
            hipMalloc((void**)&m->tab[1], sizeof(h2c_entry) * slots) == hipSuccess && hipMalloc((void**)&m->aux, sizeof(h2c_aux) * slots) == hipSuccess &&
            hipMalloc((void**)&m->row_s, sizeof(uint32_t) * slots * H2C_GRID) == hipSuccess &&
            hipMalloc((void**)&m->row_k, sizeof(uint32_t) * H2C_KEYS_MAX * H2C_GRID) == hipSuccess &&
            hipMalloc((void**)&m->ktot, sizeof(uint32_t) * (H2C_KEYS_MAX + 1u)) == hipSuccess &&
            hipMalloc((void**)&m->exp_slot, sizeof(uint32_t) * slots / 2) == hipSuccess &&
            hipMalloc((void**)&m->exp_rank, sizeof(uint32_t) * slots / 2) == hipSuccess;
  if (ok) {
    m->slots = table_slots;
    m->nmethods = nmethods;
    ok = hipMemset(m->tab[0], 0, sizeof(h2c_entry) * slots) == hipSuccess && hipMemset(m->tab[1], 0, sizeof(h2c_entry) * slots) == hipSuccess &&
         hipMemcpy(w->d, m, sizeof(h2c_dev), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    grdma_h2_calls_destroy(w);
    grdma_fail_msg(GRDMA_ERR_HIP, "h2 call table: device allocation failed");
    return nullptr;
  }
  return w;
}

// The single step and the batch share these three: the single call's arguments are one item.
// what a step of an item is refused for
static const char* h2_calls_refusal(const grdma_h2_calls_item& it) {
  if (!it.calls) return "no table";
  if (!it.d_dispatch || !it.dispatch_cap || !it.d_done || !it.done_cap || !it.d_segments || ((uintptr_t)it.d_dispatch & 15) ||
      ((uintptr_t)it.d_done & 15) || ((uintptr_t)it.d_segments & 15))
    return "a null, zero or misaligned dispatch table, done list or segment table";
  if ((it.nblocks && (!it.d_blocks || !it.d_meta)) || (it.nmsgs && !it.d_msgs) || (it.nevents && !it.d_events))
    return "a null input table with a count above 0";
  if (it.nmsgs > H2C_MSGS_MAX) return "more than 2^20 descriptors";
  if (it.nblocks >= 0xffffffffull || it.nevents >= 0xffffffffull) return "2^32 - 1 records or events, or more";
  return nullptr;
}
// the step's words of an item over its table's per-step scratch, grown to the step: a word per record, the dedup table (a
// power of two >= 2 nblocks), a record per descriptor.  false: no device memory
static bool h2_calls_call(const grdma_h2_calls_item& it, h2c_call* call) {
  grdma_h2_calls* w = it.calls;
  uint64_t dd = 64;
  while (dd < 2 * it.nblocks) dd *= 2;
  if (!h2_grow(&w->d_cls, &w->cls_cap, it.nblocks + 1) || !h2_grow(&w->d_dd, &w->dd_cap, dd) || !h2_grow(&w->d_mrec, &w->mrec_cap, it.nmsgs + 1))
    return false;
  *call = {reinterpret_cast<const h2hp_block_out*>(it.d_blocks), reinterpret_cast<const h2m_meta_out*>(it.d_meta), it.nblocks,
           reinterpret_cast<const h2c_msg*>(it.d_msgs), it.nmsgs, it.d_events, it.nevents, it.now_ns, reinterpret_cast<h2c_disp*>(it.d_dispatch),
           it.dispatch_cap, it.d_segments, reinterpret_cast<h2c_done*>(it.d_done), it.done_cap, w->d_cls, w->d_dd, dd - 1, w->d_mrec};
  return true;
}
// an item's outcome from its result words: whether its table committed; ms: what the launches took
static bool h2_calls_committed(grdma_h2_calls* w, const uint64_t* res, float ms) {
  w->ms = ms;
  return !(res[H2C_FLAGS] & H2C_F_BAD_INPUT) && !res[H2C_OVERFLOW];
}

int64_t grdma_h2_calls_step(grdma_h2_calls* w, const grdma_h2_header_block* d_blocks, const grdma_h2_call_meta* d_meta, uint64_t nblocks,
                            const grdma_h2_rx_msg* d_msgs, uint64_t nmsgs, const grdma_h2_event* d_events, uint64_t nevents, uint64_t now_ns,
                            grdma_h2_dispatch* d_dispatch, uint64_t dispatch_cap, uint32_t* d_segments, grdma_h2_call_done* d_done,
                            uint64_t done_cap, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  const char* who = "h2 call table";
  if (!w) return h2_invalid(who, "no table");
  if (!out) return h2_invalid(who, "no result array");
  const grdma_h2_calls_item it{w, d_blocks, d_meta, nblocks, d_msgs, nmsgs, d_events, nevents, now_ns, d_dispatch, dispatch_cap, d_segments, d_done, done_cap};
  if (const char* why = h2_calls_refusal(it)) return h2_invalid(who, why);
  h2_host_ctx* hc = h2_ctx();
  if (!hc) return -GRDMA_ERR_HIP;
  h2c_call call;
  if (!h2_calls_call(it, &call)) return -GRDMA_ERR_HIP;
  const h2_stage stage = h2_stage_calls(w->d);
  h2_call c{"grdma_h2_calls_step: a launch was rejected", {{w->d, &call, sizeof(call)}}, {}, {h2_all(stage)},
            {h2_result(out, w->d, offsetof(h2c_dev, res))}};
  if (int rc = h2_call_run(hc, &c)) return rc;
  if (h2_calls_committed(w, out, c.ms[0])) return (int64_t)(out[H2C_DISPATCHED] + out[H2C_ORPHANS]);
  if (out[H2C_FLAGS] & H2C_F_BAD_INPUT) return h2_invalid(who, "bad input: a request's stream id or method (the result block says which record)");
  return grdma_fail_msg(GRDMA_ERR_CAPACITY, "h2 call table: more descriptors or done records than the targets hold");
}

// The tables of many connections in the same eight launches (h2_stage_calls_links).  The batch block of the process holds
// [table | one h2c_call per item | eight result words per item] (csrc/grdma_h2_block.h): the table and the call words go
// up in ONE copy, the result words come down in ONE copy, whatever the number of items -- nothing of a step passes through
// the tables' own device blocks (F->c stays the last single step's), whose state and counters the finish launch moves
// per table as the single step does.  Every table brings its own per-step scratch.  The table follows no parser: nothing
// to wait for.  One call at a time, as the other batch calls.
int grdma_h2_calls_step_batch(const grdma_h2_calls_item* items, uint32_t n_items, uint64_t* out) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 call table batch", "table", "grdma_h2_calls_step_batch: a launch was rejected"};
  if (!items) return h2_invalid(b.who, "no item array");
  if (!out) return h2_invalid(b.who, "no result array");
  if (int rc = b.begin(true, n_items)) return rc;
  for (uint32_t i = 0; i < n_items; i++)
    if (int rc = b.item(items[i].calls, h2_calls_refusal(items[i]))) return rc;
  const h2_calls_block L = h2_calls_block_layout(sizeof(h2c_link), sizeof(h2c_call), n_items);
  if (int rc = b.reserve(L.results, L.total)) return rc;
  auto* tab = reinterpret_cast<h2c_link*>(b.up.data() + L.tab);
  auto* calls = reinterpret_cast<h2c_call*>(b.up.data() + L.calls);
  for (uint32_t i = 0; i < n_items; i++) {
    if (!h2_calls_call(items[i], &calls[i])) return -GRDMA_ERR_HIP;
    tab[i] = {items[i].calls->d, reinterpret_cast<const h2c_call*>(b.d + L.calls) + i, reinterpret_cast<uint64_t*>(b.d + L.results) + 8 * (size_t)i};
  }
  std::vector<uint64_t> down(8 * (size_t)n_items, 0);  // (out is not touched unless the call ran)
  b.c.down.push_back(h2_result(down.data(), b.d, L.results, down.size()));
  const h2_stage stage = h2_stage_calls_links(reinterpret_cast<const h2c_link*>(b.d + L.tab), n_items);
  if (int rc = b.run({h2_all(stage)})) return rc;
  memcpy(out, down.data(), down.size() * sizeof(uint64_t));
  int committed = 0;
  for (uint32_t i = 0; i < n_items; i++) committed += h2_calls_committed(items[i].calls, out + 8 * (size_t)i, b.c.ms[0]);  // (the time: the batch's, repeated)
  return committed;
}

int grdma_h2_calls_dump(grdma_h2_calls* w, void* host_buf, uint64_t cap, uint64_t out[4]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w || !out || (!host_buf && cap)) return -GRDMA_ERR_INVALID;
  h2c_dev h;
  std::vector<h2c_entry> tab(w->h.slots);
  if (!h2_read(&h, w->d, sizeof(h)) || !h2_read(tab.data(), w->h.tab[h.cur & 1u], sizeof(h2c_entry) * tab.size())) return -GRDMA_ERR_HIP;
  std::vector<h2c_entry> live;
  for (h2c_entry e : tab) {
    if (e.stream == 0 || (e.fin & H2C_EF_DEAD)) continue;
    e.word |= e.fin;
    e.fin = 0;
    e.pad1 = 0;
    live.push_back(e);
  }
  std::sort(live.begin(), live.end(), [](const h2c_entry& a, const h2c_entry& b) { return a.stream < b.stream; });
  out[0] = live.size();
  out[1] = live.size() * sizeof(h2c_entry);
  out[2] = h.serial;
  out[3] = w->h.slots;
  if (out[1] > cap) return -GRDMA_ERR_CAPACITY;
  if (!live.empty()) memcpy(host_buf, live.data(), out[1]);
  return 0;
}

int grdma_h2_calls_stats(grdma_h2_calls* w, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!w || !out) return -GRDMA_ERR_INVALID;
  h2c_dev h;
  if (!h2_read(&h, w->d, sizeof(h))) return -GRDMA_ERR_HIP;
  out[0] = h.st_steps, out[1] = h.st_opened, out[2] = h.st_msgs, out[3] = h.st_bytes, out[4] = h.st_orphans, out[5] = h.st_done;
  out[6] = h.lost ? GRDMA_H2_CALLS_LOST : 0;
  out[7] = (uint64_t)(w->ms * 1e6f);
  return 0;
}

// ---- the message assembler on many links (h2_stage_asm_links, csrc/grdma_h2_asm.h) ---------------------------------
namespace {
// the pinned table of grdma_h2_asm_release_batch with the event of its last upload (the table is reused: the next call
// waits for that upload)
struct h2_links_ctx {
  hipEvent_t rel_up = nullptr;
  h2a_link_release* h_rel = nullptr;
  h2a_link_release* d_rel = nullptr;
  bool rel_pending = false;
};
h2_links_ctx* h2_links() {
  static h2_links_ctx c;
  static const bool ok = hipEventCreateWithFlags(&c.rel_up, hipEventDisableTiming) == hipSuccess &&
                         hipHostMalloc((void**)&c.h_rel, sizeof(h2a_link_release) * GRDMA_H2_BATCH_MAX) == hipSuccess &&
                         hipMalloc((void**)&c.d_rel, sizeof(h2a_link_release) * GRDMA_H2_BATCH_MAX) == hipSuccess;
  return ok ? &c : nullptr;
}
}  // namespace

int grdma_h2_deframe_messages_batch(grdma_h2_messages_item* items, uint32_t n_items) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  h2_batch b{"h2 messages batch", "parser", "h2 messages batch: a launch was rejected"};
  if (int rc = b.begin(items, n_items)) return rc;
  uint64_t n_sl = 0, n_ev = 0;
  bool want_events = false;
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_messages_item& it = items[i];
    const char* why = nullptr;
    if (!it.parser || !it.d_arena || (!it.slices && it.n) || it.cap == 0 || (!it.msgs_out && it.msgs_cap))
      why = "an item without parser, arena, slices, event capacity or descriptor array";
    else if (!it.assembler) why = "an item without assembler";
    else if (it.assembler->parser != it.parser) why = "an assembler of another parser";
    else if (it.parser->fc) why = "a parser with a flow-control ledger (single transport only)";
    else if (it.assembler->attached || it.parser->asm_attached) why = "an assembler attached to a pipe";
    if (int rc = b.item(it.parser, why)) return rc;  // (an assembler has one parser: its items are distinct with their parsers)
    n_sl += it.n;
    n_ev += it.cap;
    want_events = want_events || it.events_out;
  }
  for (uint32_t i = 0; i < n_items; i++)
    if (!h2_asm_prepare(items[i].assembler, items[i].cap)) return -GRDMA_ERR_HIP;
  const h2_deframe_block L = h2_deframe_batch_layout(n_items, n_sl, n_ev, true);
  if (int rc = b.reserve(L.events, L.total)) return rc;  // ([0, events) goes up)
  hipStream_t st = b.hc->stream;
  uint8_t* const d = b.d;
  // (the events come down only when an item asks for them)
  std::vector<uint8_t> down((want_events ? L.total : L.events) - L.results);
  h2_batch_pack(items, n_items, L, b.up.data(), d);
  // on top of the deframe table: every assembler with a call block that names what its item's deframer leaves
  const auto* dtab = reinterpret_cast<const grdma_h2_link_deframe*>(b.up.data() + L.tab);
  auto* atab = reinterpret_cast<h2a_link*>(b.up.data() + L.asm_tab);
  auto* calls = reinterpret_cast<h2a_call*>(b.up.data() + L.asm_calls);
  for (uint32_t i = 0; i < n_items; i++) {
    const grdma_h2_link_deframe& q = dtab[i];
    calls[i] = h2a_call{q.ev, q.res, q.slices, q.arena, q.ev_cap, 0};
    atab[i].A = items[i].assembler->d;
    atab[i].call = reinterpret_cast<const h2a_call*>(d + L.asm_calls) + i;
    b.behind.push_back(items[i].parser);
  }
  // the deframing; then the assembly: the plan and the copy, timed apart.  One download of the results (and the events);
  // then every assembler's block, and below the descriptors from where each assembler keeps them (its own buffer: the
  // kernels are the single call's, which reports from there)
  const h2_stage deframing = h2_stage_deframe_links(reinterpret_cast<const grdma_h2_link_deframe*>(d + L.tab), n_items);
  const h2_stage assembly = h2_stage_asm_links(reinterpret_cast<const h2a_link*>(d + L.asm_tab), n_items);
  std::vector<h2a_dev> hs(n_items);
  b.c.down.push_back({down.data(), d + L.results, down.size()});
  for (uint32_t i = 0; i < n_items; i++) b.c.down.push_back({&hs[i], items[i].assembler->d, sizeof(h2a_dev)});
  if (int rc = b.run({h2_all(deframing), h2_asm_plan(assembly), h2_asm_copy(assembly)})) return rc;
  const h2_call& c = b.c;
  g_h2_last_kernel_us = 1e3 * c.ms[0];
  h2_batch_hand_back(items, n_items, L, down.data());
  bool more = false;
  for (uint32_t i = 0; i < n_items; i++) {
    grdma_h2_messages_item& it = items[i];
    it.assembler->plan_ms = c.ms[1];  // (the batch's, repeated)
    it.assembler->copy_ms = c.ms[2];
    it.assembler->calls++;
    it.n_msgs = it.n_events < 0 ? -(int64_t)GRDMA_ERR_CAPACITY : h2_asm_descriptors(hs[i], it.msgs_out, it.msgs_cap, st);
    if (it.n_msgs == -(int64_t)GRDMA_ERR_HIP) return -GRDMA_ERR_HIP;
    more = more || it.n_msgs > 0;
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
  return h2_launch(&release, 1, st) == hipSuccess ? 0 : h2_refused(st, "h2 release batch: the launch was rejected");
}
