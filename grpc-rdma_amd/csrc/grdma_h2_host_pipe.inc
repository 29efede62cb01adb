// HTTP/2 inside the device pipeline: the pipes.  Included by csrc/grdma_h2.hip (inside its extern "C" block), behind the
// stage builders, the parser, the assembler and the reply.
//
// A step of a pipe is  frame -> the streaming job -> deframe [-> assemble], all enqueued.  The framing stage rebuilds the
// job's slice list from a message table (a reply pipe: from the descriptors a forward pipe assembled), the deframing
// stage parses the slices the job delivered.  By default the stages are kernel nodes of the job's own graph, one launch
// per step: a graph boundary costs ~15-20 us of idle device on each side.  With GRDMA_H2_PIPE_FUSED=0 the same stage
// lists are launched around the job's launch, ordered by events, with per-stage event timing.
//
// The single pipe (grdma_h2_pipe) does this for one link of a job; the group pipe (grdma_h2_group_pipe) for many links
// of ONE job with one kernel per stage.  What a step waits for and what it leaves for the next one is the same for both:
// they embed one h2_step_seq, and h2_seq_enqueue is the only place that knows the order.
struct grdma_stream_job;
int grdma_job_link_view(grdma_stream_job* j, uint32_t link, grdma_sge** d_sges, uint64_t* count,
                        grdma_slice_out** d_slices, uint8_t** dst, hipStream_t* stream);
extern "C" uint32_t grdma_job_link_count(grdma_stream_job* j);
extern "C" int grdma_job_link_step_slices(grdma_stream_job* j, uint32_t link, const uint64_t** d_count, uint64_t* cap);
int grdma_stream_job_launch(grdma_stream_job* j);
extern "C" int grdma_job_set_hooks(grdma_stream_job* j, const grdma_job_hook* pre, uint32_t n_pre, const grdma_job_hook* post,
                                   uint32_t n_post);
extern "C" int grdma_job_hook_counts(grdma_stream_job* j, uint32_t out[2]);

// ---- the step sequencer ------------------------------------------------------------------------------------------------
struct h2_step_seq {
  grdma_stream_job* job = nullptr;
  hipStream_t job_stream = nullptr, frame_stream = nullptr, deframe_stream = nullptr;
  hipEvent_t framed = nullptr, job_done = nullptr, deframed = nullptr;
  hipEvent_t t_f0 = nullptr, t_f1 = nullptr, t_d0 = nullptr, t_d1 = nullptr;  // kernel start / end stamps of the last step
  bool launched = false;
  bool fused = false;  // the stages are nodes of the job's graph (one launch per step)
  bool timed = false;  // the last step recorded the per-stage timing events
  h2_stage pre, post;  // the framing stage; the deframing stage with, behind it, the attached assemblers'
  std::vector<grdma_h2_parser*> parsers;  // the step deframes with these: one per link of the pipe
  std::vector<grdma_h2_reply*> replies;   // a reply pipe: the step frames from these, one per link
  std::vector<grdma_h2_asm*> asms;        // the step assembles into these: empty, or one entry per link (NULL = none)
  std::vector<grdma_h2_fc*> fcs;          // the window ledgers that account every step's events: empty, or one entry per link (NULL = none)
};

namespace {
hipStream_t g_pipe_frame_stream = nullptr, g_pipe_deframe_stream = nullptr;
}

// The streams the pipes share and the events of one pipe.  The caller sets job_stream (grdma_job_link_view) and
// deframe_stream.
static bool h2_seq_create(h2_step_seq* s, grdma_stream_job* job) {
  if (!g_pipe_frame_stream &&
      (hipStreamCreateWithFlags(&g_pipe_frame_stream, hipStreamNonBlocking) != hipSuccess ||
       hipStreamCreateWithFlags(&g_pipe_deframe_stream, hipStreamNonBlocking) != hipSuccess))
    return false;
  s->job = job;
  s->frame_stream = g_pipe_frame_stream;  // shared by all pipes: framings are ordered among themselves
  return hipEventCreateWithFlags(&s->framed, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&s->job_done, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&s->deframed, hipEventDisableTiming) == hipSuccess &&
         hipEventCreate(&s->t_f0) == hipSuccess && hipEventCreate(&s->t_f1) == hipSuccess &&
         hipEventCreate(&s->t_d0) == hipSuccess && hipEventCreate(&s->t_d1) == hipSuccess;
}

// The two stages of a step: nodes of the job's own graph by default, with GRDMA_H2_PIPE_FUSED=0 kept for
// h2_seq_enqueue to launch around the job.
static bool h2_seq_install(h2_step_seq* s, const h2_stage& pre, const h2_stage& post) {
  s->pre = pre;
  s->post = post;
  const char* fe = getenv("GRDMA_H2_PIPE_FUSED");
  if (fe && atoi(fe) == 0) return true;
  if (grdma_job_set_hooks(s->job, pre.data(), (uint32_t)pre.size(), post.data(), (uint32_t)post.size()) != 0) return false;
  s->fused = true;
  s->deframe_stream = s->job_stream;
  return true;
}

// A reply pipe's step frames one link from r: the link's framer writes the link's slice table, and only a reply of the
// shape the job's graph was recorded for.  The source of a reply pipe assembles in forward pipes.
static bool h2_seq_bind_reply(h2_step_seq* s, grdma_h2_reply* r, grdma_sge* d_sges, uint64_t count, uint8_t* d_hdr,
                              uint64_t hdr_cap, uint64_t recorded_wire_bytes) {
  if (r->seq || !r->src->attached || r->d_wr) return false;  // (a reply under send windows frames standalone only)
  if (!h2_reply_set_target(r, d_sges, count, d_hdr, hdr_cap, 1, count, recorded_wire_bytes, nullptr)) return false;
  r->seq = s;
  r->src->reply_pipes++;
  s->replies.push_back(r);
  return true;
}

// One more stage behind what the step runs behind the job already -- the deframing stage and whatever was attached
// before (fused: the job's graph is rebuilt with it).  Stages stand in the order they were attached in.
static int h2_seq_append(h2_step_seq* s, const h2_stage& stage) {
  h2_stage post = s->post;
  post.insert(post.end(), stage.begin(), stage.end());
  if (s->fused &&
      grdma_job_set_hooks(s->job, s->pre.data(), (uint32_t)s->pre.size(), post.data(), (uint32_t)post.size()) != 0)
    return -GRDMA_ERR_HIP;
  s->post = post;
  return 0;
}

// The assemblers' stage goes behind the deframing stage; from now on a step assembles into asms, one entry per parser
// of the pipe (NULL = none).
static int h2_seq_attach(h2_step_seq* s, const h2_stage& assembly, grdma_h2_asm* const* asms, uint32_t n) {
  if (int rc = h2_seq_append(s, assembly)) return rc;
  s->asms.assign(asms, asms + n);
  for (grdma_h2_asm* a : s->asms)
    if (a) {
      a->attached++;
      a->parser->asm_attached++;
    }
  return 0;
}

// everything the pipe enqueued has ended
static int h2_seq_wait(const h2_step_seq* s) {
  if (hipStreamSynchronize(s->frame_stream) != hipSuccess || hipStreamSynchronize(s->job_stream) != hipSuccess ||
      (s->deframe_stream != s->job_stream && hipStreamSynchronize(s->deframe_stream) != hipSuccess))
    return -GRDMA_ERR_HIP;
  return 0;
}

// every parser's state is handed over from its previous deframing (a pipe step or a call on another stream)
static bool h2_seq_wait_parsers(const h2_step_seq* s, hipStream_t st) {
  for (const grdma_h2_parser* p : s->parsers)
    if (!h2_wait_parser(st, p)) return false;
  return true;
}
// a reply step reads what the forward steps assembled: behind every distinct source parser's last deframing
static bool h2_seq_wait_sources(const h2_step_seq* s, hipStream_t st) {
  for (size_t i = 0; i < s->replies.size(); i++) {
    const grdma_h2_parser* fp = s->replies[i]->src->parser;
    bool seen = false;
    for (size_t k = 0; k < i && !seen; k++) seen = s->replies[k]->src->parser == fp;
    if (!seen && !h2_wait_parser(st, fp)) return false;
  }
  return true;
}
// a step's release (at the start of its assembly) waits for the last reply step that still gathers from the arena
static bool h2_seq_wait_readers(const h2_step_seq* s) {
  for (const grdma_h2_asm* a : s->asms)
    if (a && a->last_read && hipStreamWaitEvent(s->job_stream, a->last_read, 0) != hipSuccess) return false;
  return true;
}

// One step, enqueued.  Fused it is one graph launch: the framing stage -> the job's rounds -> the deframing stage
// [-> the assemblers']; steps and pipes of one connection are ordered by the job's stream.  Unfused the framing stage
// runs on the frame stream and the deframing stage on the deframe stream (the job's, unless the single pipe was given
// one of its own), tied to the job's launch by events; d_fres / fres_bytes: the framing results, zeroed in front.
//
// The ordering rules, each of them here and nowhere else:
//  * a parser's state is handed from one deframing to the next: the stream that deframes waits for last_deframed of
//    every parser of the step, and the step leaves its own event there;
//  * a reply step frames behind the last deframing (and so the assembly) of every source's forward parser;
//  * an assembler's release, the first thing its stage does, goes behind the last reply step that gathers from its
//    arena (last_read).  That wait is on the job's stream in front of the job's launch in both modes: unfused too the
//    assembly is behind it, because the deframe stream waits for job_done.  (The unfused single pipe used to put it on
//    the deframe stream behind the deframer; same results, one place less.)
static int h2_seq_enqueue(h2_step_seq* s, void* d_fres, size_t fres_bytes) {
  const hipStream_t js = s->job_stream, fs = s->frame_stream, ds = s->deframe_stream;  // (fused: ds == js)
  s->timed = !s->fused;
  if (s->fused) {
    if (!h2_seq_wait_parsers(s, js) || !h2_seq_wait_sources(s, js)) return -GRDMA_ERR_HIP;
  } else {
    // framing overwrites the slice table the job's previous step read
    if (s->launched && hipStreamWaitEvent(fs, s->job_done, 0) != hipSuccess) return -GRDMA_ERR_HIP;
    if (hipMemsetAsync(d_fres, 0, fres_bytes, fs) != hipSuccess) return -GRDMA_ERR_HIP;
    if (!h2_seq_wait_sources(s, fs)) return -GRDMA_ERR_HIP;
    hipEventRecord(s->t_f0, fs);
    if (h2_launch(s->pre, fs) != hipSuccess) return -GRDMA_ERR_HIP;
    hipEventRecord(s->t_f1, fs);
    if (hipEventRecord(s->framed, fs) != hipSuccess) return -GRDMA_ERR_HIP;
    // the job reads the slice table and overwrites what the previous deframing parsed
    if (hipStreamWaitEvent(js, s->framed, 0) != hipSuccess) return -GRDMA_ERR_HIP;
    if (s->launched && ds != js && hipStreamWaitEvent(js, s->deframed, 0) != hipSuccess) return -GRDMA_ERR_HIP;
  }
  if (!h2_seq_wait_readers(s)) return -GRDMA_ERR_HIP;
  const int rc = grdma_stream_job_launch(s->job);
  if (rc < 0) return rc;
  if (!s->fused) {
    if (hipEventRecord(s->job_done, js) != hipSuccess) return -GRDMA_ERR_HIP;
    for (grdma_h2_reply* r : s->replies) r->src->last_read = s->job_done;  // (the job's gather from the sources' arenas ends here)
    if (ds != js && hipStreamWaitEvent(ds, s->job_done, 0) != hipSuccess) return -GRDMA_ERR_HIP;
    if (!h2_seq_wait_parsers(s, ds)) return -GRDMA_ERR_HIP;
    hipEventRecord(s->t_d0, ds);
    if (h2_launch(s->post, ds) != hipSuccess) return -GRDMA_ERR_HIP;
    hipEventRecord(s->t_d1, ds);
  }
  if (hipEventRecord(s->deframed, ds) != hipSuccess) return -GRDMA_ERR_HIP;
  // what the step leaves for the next: (fused) the end of the graph as the end of the job's gather, and the parsers' state
  if (s->fused)
    for (grdma_h2_reply* r : s->replies) r->src->last_read = s->deframed;
  for (grdma_h2_parser* p : s->parsers) {
    p->last_stream = ds;
    p->last_deframed = s->deframed;
  }
  s->launched = true;
  return 0;
}

// a reply pipe's job gathers from an arena this pipe assembles into: that pipe is destroyed first
static bool h2_seq_read_by_reply_pipes(const h2_step_seq* s) {
  for (const grdma_h2_asm* a : s->asms)
    if (a && a->reply_pipes != 0) return true;
  return false;
}

// The end of a pipe: its steps are waited for, then nothing points at its events any more, the job's graph runs
// without its stages, and its replies and assemblers are free again.
static void h2_seq_destroy(h2_step_seq* s) {
  if (s->launched) h2_seq_wait(s);
  for (grdma_h2_parser* p : s->parsers)
    if (p->last_deframed == s->deframed) p->last_deframed = nullptr;
  if (s->fused && s->job) grdma_job_set_hooks(s->job, nullptr, 0, nullptr, 0);
  for (grdma_h2_reply* r : s->replies) {
    if (r->src->last_read == s->deframed || r->src->last_read == s->job_done) r->src->last_read = nullptr;
    r->src->reply_pipes--;
    r->seq = nullptr;
  }
  s->replies.clear();
  for (grdma_h2_asm* a : s->asms)
    if (a) {
      a->parser->asm_attached--;
      a->attached--;
    }
  s->asms.clear();
  for (grdma_h2_fc* f : s->fcs)
    if (f) f->seq = nullptr;
  s->fcs.clear();
  for (hipEvent_t e : {s->framed, s->job_done, s->deframed, s->t_f0, s->t_f1, s->t_d0, s->t_d1})
    if (e) hipEventDestroy(e);
}

// kernel time of the two stages of the last step, microseconds (0 for a fused step: nothing stamps inside a graph)
static void h2_seq_stage_us(const h2_step_seq* s, uint64_t* f_us, uint64_t* d_us) {
  float fms = 0, dms = 0;
  *f_us = *d_us = 0;
  if (s->launched && s->timed && hipEventElapsedTime(&fms, s->t_f0, s->t_f1) == hipSuccess) *f_us = (uint64_t)(fms * 1e3f);
  if (s->launched && s->timed && hipEventElapsedTime(&dms, s->t_d0, s->t_d1) == hipSuccess) *d_us = (uint64_t)(dms * 1e3f);
}

// The report of one link's step: {slices framed, frame overflow, events, deframe overflow, slices parsed, h2 error,
// framing kernel us, deframing kernel us, bulk steps, frames parsed by bulk steps, then the deframer's device-clock
// ticks: waiting for the look-ahead ring, in bulk steps, total, in the byte-wise path}
static void h2_step_report(uint64_t out[14], const grdma_h2_frame_result& fr, const grdma_h2_deframe_result& dr, uint64_t f_us,
                           uint64_t d_us) {
  out[0] = fr.nslices;
  out[1] = fr.overflow;
  out[2] = dr.nevents;
  out[3] = dr.overflow;
  out[4] = dr.slices_done;
  out[5] = (uint64_t)dr.error;
  out[6] = f_us;
  out[7] = d_us;
  out[8] = dr.bulk_steps;
  out[9] = dr.bulk_frames;
  out[10] = dr.t_wait;
  out[11] = dr.t_bulk;
  out[12] = dr.t_total;
  out[13] = dr.t_serial;
}

// the messages the last step assembled into a (its assembly ends with the step)
static int64_t h2_seq_messages(const h2_step_seq* s, const grdma_h2_asm* a, grdma_h2_rx_msg* out, uint64_t cap) {
  if (int rc = h2_seq_wait(s)) return rc;
  h2a_dev h;
  if (hipMemcpy(&h, a->d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -GRDMA_ERR_HIP;
  return h2_asm_descriptors(h, out, cap, nullptr);
}

// ---- one link of a job (the single pipe) -------------------------------------------------------------------------------
// It can deframe over chunks, frame more than H2_FRAME_ONE_MAX messages, and have a deframe stream of its own.
struct grdma_h2_pipe {
  h2_step_seq seq;  // one parser; at most one reply and one assembler
  grdma_sge* d_sges = nullptr;
  uint64_t count = 0;
  grdma_slice_out* d_slices = nullptr;
  uint8_t* dst = nullptr;
  grdma_h2_msg_dev* d_msgs = nullptr;
  grdma_h2_msg_pos* d_pos = nullptr;
  uint8_t* d_hdr = nullptr;
  uint64_t hdr_cap = 0;
  grdma_h2_frame_result* d_fres = nullptr;
  grdma_h2_deframe_result* d_dres = nullptr;
  grdma_h2_event* d_ev = nullptr;
  uint64_t ev_cap = 0;
  uint64_t boundary_steps = 0, t_boundary = 0;  // of the last synced step
  h2a_call* d_call = nullptr;  // where this pipe's deframer leaves its output, for the assembler
  // the window ledger's call block and the window-update list of a step (grdma_h2_pipe_attach_flow_control)
  h2fc_call* d_fc_call = nullptr;
  grdma_sge* d_wu = nullptr;
  uint8_t* d_wu_hdr = nullptr;
  uint64_t wu_cap = 0;
};

// msgs / nmsgs / max_frame: the host message table of grdma_h2_pipe_create; reply: the framing stage of
// grdma_h2_pipe_create_reply instead (no message table of its own: the reply's plan builds one per step)
static grdma_h2_pipe* h2_pipe_create(grdma_stream_job* job, uint32_t link, const grdma_h2_msg* msgs, uint64_t nmsgs,
                                     uint32_t max_frame, grdma_h2_parser* parser, uint64_t delivered_slices,
                                     uint64_t events_cap, grdma_h2_reply* reply, uint64_t recorded_wire_bytes) {
  if (grdma_device_count() <= 0 || !job || !parser) return nullptr;
  if (!reply && (!msgs || !nmsgs || max_frame == 0 || max_frame >= (1u << 24))) return nullptr;
  grdma_h2_pipe* p = new grdma_h2_pipe();
  h2_step_seq& s = p->seq;
  s.parsers.push_back(parser);
  p->ev_cap = events_cap;
  bool ok = h2_seq_create(&s, job) &&
            grdma_job_link_view(job, link, &p->d_sges, &p->count, &p->d_slices, &p->dst, &s.job_stream) == 0;
  // The deframing goes behind the job on the JOB's stream unless GRDMA_H2_DEFRAME_STREAM=1 asks for a stream of its
  // own (shared by all pipes): the next job does not start before the deframing has ended either way (measured: kernels
  // of the two streams do not run side by side), and a hand-over between streams costs ~20 us of idle device on each
  // side of it.
  static const bool own_stream = [] { const char* e = getenv("GRDMA_H2_DEFRAME_STREAM"); return e && atoi(e) != 0; }();
  s.deframe_stream = own_stream ? g_pipe_deframe_stream : s.job_stream;
  p->hdr_cap = 32 * (p->count + 64);
  ok = ok && (reply || (h2_upload_msgs(msgs, nmsgs, &p->d_msgs) &&
                        hipMalloc((void**)&p->d_pos, sizeof(grdma_h2_msg_pos) * nmsgs) == hipSuccess)) &&
       hipMalloc((void**)&p->d_hdr, p->hdr_cap) == hipSuccess &&
       hipMalloc((void**)&p->d_fres, sizeof(grdma_h2_frame_result)) == hipSuccess &&
       hipMalloc((void**)&p->d_dres, sizeof(grdma_h2_deframe_result)) == hipSuccess &&
       hipMalloc((void**)&p->d_ev, sizeof(grdma_h2_event) * (events_cap ? events_cap : 1)) == hipSuccess &&
       (!reply || h2_seq_bind_reply(&s, reply, p->d_sges, p->count, p->d_hdr, p->hdr_cap, recorded_wire_bytes));
  if (ok) {
    const bool chunked = delivered_slices >= H2_CHUNK_MIN_SLICES && h2_chunks_prepare(parser, events_cap, s.deframe_stream);
    ok = h2_seq_install(&s,
                        reply ? h2_stage_reply(reply->d)
                              : h2_stage_frame(p->d_msgs, nmsgs, max_frame, p->d_sges, p->count, p->d_hdr, p->hdr_cap, p->d_pos, p->d_fres),
                        h2_stage_deframe(parser, p->dst, p->d_slices, delivered_slices, p->d_ev, events_cap, p->d_dres, chunked));
  }
  if (!ok) {
    grdma_h2_pipe_destroy(p);
    return nullptr;
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
  if (!p || h2_seq_read_by_reply_pipes(&p->seq)) return;
  h2_seq_destroy(&p->seq);
  hipFree(p->d_call);
  hipFree(p->d_fc_call);
  hipFree(p->d_wu);
  hipFree(p->d_wu_hdr);
  hipFree(p->d_msgs);
  hipFree(p->d_pos);
  hipFree(p->d_hdr);
  hipFree(p->d_fres);
  hipFree(p->d_dres);
  hipFree(p->d_ev);
  delete p;
}

// One step on the job's captured graph (schedule 0: the only schedule since the link engine was retired).
int grdma_h2_pipe_enqueue(grdma_h2_pipe* p, int schedule) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || schedule != 0) return -GRDMA_ERR_INVALID;
  return h2_seq_enqueue(&p->seq, p->d_fres, sizeof(grdma_h2_frame_result));
}

// Wait for the last step and report it (h2_step_report); events_out (may be NULL) receives up to cap events.
int grdma_h2_pipe_sync(grdma_h2_pipe* p, uint64_t out[14], grdma_h2_event* events_out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !out) return -GRDMA_ERR_INVALID;
  if (int rc = h2_seq_wait(&p->seq)) return rc;
  grdma_h2_frame_result fr;
  grdma_h2_deframe_result dr;
  if (hipMemcpy(&fr, p->d_fres, sizeof(fr), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&dr, p->d_dres, sizeof(dr), hipMemcpyDeviceToHost) != hipSuccess)
    return -GRDMA_ERR_HIP;
  // (a reply's overflow 2: the step had another shape than the recorded one)
  if (!p->seq.replies.empty() && !h2_reply_result(p->seq.replies[0], &fr)) return -GRDMA_ERR_HIP;
  uint64_t f_us, d_us;
  h2_seq_stage_us(&p->seq, &f_us, &d_us);
  h2_step_report(out, fr, dr, f_us, d_us);
  p->boundary_steps = dr.boundary_steps;
  p->t_boundary = dr.t_boundary;
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

int64_t grdma_h2_pipe_slice_table(grdma_h2_pipe* p, grdma_slice* out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || (!out && cap)) return -GRDMA_ERR_INVALID;
  if (p->count > cap) return -GRDMA_ERR_CAPACITY;
  static_assert(sizeof(grdma_slice) == sizeof(grdma_sge), "layout");
  if (int rc = h2_seq_wait(&p->seq)) return rc;
  if (p->count && hipMemcpy(out, p->d_sges, sizeof(grdma_sge) * p->count, hipMemcpyDeviceToHost) != hipSuccess) return -GRDMA_ERR_HIP;
  return (int64_t)p->count;
}

int grdma_h2_pipe_attach_assembler(grdma_h2_pipe* p, grdma_h2_asm* a) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !a || a->parser != p->seq.parsers[0] || !p->seq.asms.empty()) return -GRDMA_ERR_INVALID;
  if (p->seq.launched && h2_seq_wait(&p->seq) != 0) return -GRDMA_ERR_HIP;
  if (!h2_asm_prepare(a, p->ev_cap ? p->ev_cap : 1)) return -GRDMA_ERR_HIP;
  // (a step first releases everything reported before it)
  const h2a_call call{p->d_ev, p->d_dres, p->d_slices, p->dst, p->ev_cap, 1};
  if (!p->d_call && hipMalloc((void**)&p->d_call, sizeof(h2a_call)) != hipSuccess) return -GRDMA_ERR_HIP;
  if (hipMemcpy(p->d_call, &call, sizeof(call), hipMemcpyHostToDevice) != hipSuccess) return -GRDMA_ERR_HIP;
  return h2_seq_attach(&p->seq, h2_stage_asm(a->d, p->d_call), &a, 1);
}

int64_t grdma_h2_pipe_messages(grdma_h2_pipe* p, grdma_h2_rx_msg* out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || p->seq.asms.empty() || (!out && cap)) return -GRDMA_ERR_INVALID;
  return h2_seq_messages(&p->seq, p->seq.asms[0], out, cap);
}

// The window ledger's stage goes behind what the pipe runs behind its job at the time of the call: behind the deframer,
// and behind the assembler's six kernels if that was attached first (in front of them if it comes later).  It reads the
// events only, so either order gives the same bytes.  The pipe owns the window-update list: room for max_updates frames.
int grdma_h2_pipe_attach_flow_control(grdma_h2_pipe* p, grdma_h2_fc* f) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !f) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 pipe: a pipe and a ledger");
  if (!p->seq.replies.empty()) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 pipe: a reply pipe carries no window ledger (not built)");
  if (!p->seq.fcs.empty()) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 pipe: a ledger is attached already");
  if (f->seq) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 pipe: the ledger is attached to another pipe");
  if (!f->parser) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 pipe: the ledger's parser is gone");
  if (f->parser != p->seq.parsers[0]) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 pipe: the ledger of another parser than the pipe's");
  h2_host_ctx* hc = h2_ctx();
  if (!hc || hipStreamSynchronize(hc->stream) != hipSuccess) return -GRDMA_ERR_HIP;  // (the ledger's standalone calls)
  if (p->seq.launched && h2_seq_wait(&p->seq) != 0) return -GRDMA_ERR_HIP;
  if (!h2_fc_prepare(f, p->ev_cap)) return -GRDMA_ERR_HIP;
  p->wu_cap = (f->h.max_updates * H2FC_FRAME + H2_INLINED - 1) / H2_INLINED;
  const h2fc_call call{p->d_ev, p->d_dres, p->ev_cap};
  if ((!p->d_fc_call && hipMalloc((void**)&p->d_fc_call, sizeof(h2fc_call)) != hipSuccess) ||
      (!p->d_wu && hipMalloc((void**)&p->d_wu, sizeof(grdma_sge) * p->wu_cap) != hipSuccess) ||
      (!p->d_wu_hdr && hipMalloc((void**)&p->d_wu_hdr, 32 * p->wu_cap) != hipSuccess) ||
      hipMemcpy(p->d_fc_call, &call, sizeof(call), hipMemcpyHostToDevice) != hipSuccess ||
      !h2_fc_set_target(f, p->d_wu, p->wu_cap, p->d_wu_hdr, 32 * p->wu_cap, nullptr))
    return -GRDMA_ERR_HIP;
  if (int rc = h2_seq_append(&p->seq, h2_stage_fc(f->d, p->d_fc_call))) return rc;
  p->seq.fcs.assign(1, f);
  f->seq = &p->seq;
  return 0;
}

// The window-update list a ledger left in a pipe's tables (d_wu, d_wu_hdr) in the last step, after the enqueued steps
// have ended: the readers of the single pipe and, per link, of the group pipe.
static int h2_seq_wu_result(const h2_step_seq* s, const grdma_h2_fc* f, uint64_t res[8]) {
  if (int rc = h2_seq_wait(s)) return rc;
  if (hipMemcpy(res, reinterpret_cast<const uint8_t*>(f->d) + offsetof(h2fc_dev, res), 8 * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
    return -GRDMA_ERR_HIP;
  return 0;
}
static int64_t h2_seq_window_updates(const h2_step_seq* s, const grdma_h2_fc* f, const grdma_sge* d_wu, grdma_slice* slices_out,
                                     uint64_t cap, uint64_t out[8]) {
  if (int rc = h2_seq_wu_result(s, f, out)) return rc;
  if (out[H2FC_OVERFLOW]) return -GRDMA_ERR_CAPACITY;
  const uint64_t n = out[H2FC_SLICES];
  if (n > cap) return -GRDMA_ERR_CAPACITY;
  static_assert(sizeof(grdma_slice) == sizeof(grdma_sge), "layout");
  if (n && hipMemcpy(slices_out, d_wu, sizeof(grdma_sge) * n, hipMemcpyDeviceToHost) != hipSuccess) return -GRDMA_ERR_HIP;
  return (int64_t)n;
}
static int64_t h2_seq_window_update_bytes(const h2_step_seq* s, const grdma_h2_fc* f, const uint8_t* d_wu_hdr, void* bytes_out,
                                          uint64_t cap) {
  uint64_t res[8];
  if (int rc = h2_seq_wu_result(s, f, res)) return rc;
  if (res[H2FC_OVERFLOW] || res[H2FC_WIRE] > cap) return -GRDMA_ERR_CAPACITY;
  const uint64_t n = res[H2FC_SLICES];
  std::vector<uint8_t> arena(32 * n);
  if (n && hipMemcpy(arena.data(), d_wu_hdr, arena.size(), hipMemcpyDeviceToHost) != hipSuccess) return -GRDMA_ERR_HIP;
  uint8_t* dst = static_cast<uint8_t*>(bytes_out);
  uint64_t done = 0;
  for (uint64_t k = 0; k < n; k++) {  // (slice k holds wire bytes [23 k, 23 k + 23) at arena + 32 k)
    const uint64_t len = std::min<uint64_t>(H2_INLINED, res[H2FC_WIRE] - done);
    memcpy(dst + done, arena.data() + 32 * k, len);
    done += len;
  }
  return (int64_t)done;
}

int64_t grdma_h2_pipe_window_updates(grdma_h2_pipe* p, grdma_slice* slices_out, uint64_t cap, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || p->seq.fcs.empty() || !out || (!slices_out && cap)) return -GRDMA_ERR_INVALID;
  return h2_seq_window_updates(&p->seq, p->seq.fcs[0], p->d_wu, slices_out, cap, out);
}

int64_t grdma_h2_pipe_window_update_bytes(grdma_h2_pipe* p, void* bytes_out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || p->seq.fcs.empty() || (!bytes_out && cap)) return -GRDMA_ERR_INVALID;
  return h2_seq_window_update_bytes(&p->seq, p->seq.fcs[0], p->d_wu_hdr, bytes_out, cap);
}

// ---- several links of ONE job (the group pipe) ---------------------------------------------------------------------
// A job carries one set of hooks (grdma_job_set_hooks assigns): the stages of all listed links are ONE framing kernel
// over a table of links in front of the job and ONE deframing kernel behind it -- one launch per step however many
// links.  Links that are not listed keep their tables and are carried as before.  Unlike the single pipe it refuses a
// job that already carries hooks, and takes each link's step slice count from the device.
struct h2_group_link {
  grdma_sge* d_sges = nullptr;
  uint64_t count = 0;
  grdma_slice_out* d_slices = nullptr;
  uint8_t* dst = nullptr;
  grdma_h2_msg_dev* d_msgs = nullptr;
  uint8_t* d_hdr = nullptr;
  uint64_t hdr_cap = 0;
  grdma_h2_event* d_ev = nullptr;
  uint64_t ev_cap = 0;
  // the window-update list of a step, for a link with a ledger (grdma_h2_group_pipe_attach_flow_control)
  grdma_sge* d_wu = nullptr;
  uint8_t* d_wu_hdr = nullptr;
  uint64_t wu_cap = 0;
};
struct grdma_h2_group_pipe {
  h2_step_seq seq;  // one parser per listed link; a group reply pipe: one reply per listed link
  std::vector<h2_group_link> links;
  grdma_h2_link_frame* d_ftab = nullptr;
  h2r_link* d_rtab = nullptr;  // a group reply pipe (grdma_h2_group_pipe_create_reply): the framers of the links
  grdma_h2_link_deframe* d_dtab = nullptr;
  grdma_h2_frame_result* d_fres = nullptr;    // one per listed link
  grdma_h2_deframe_result* d_dres = nullptr;  // one per listed link
  h2a_link* d_atab = nullptr;   // the links with an assembler, in spec order (grdma_h2_group_pipe_attach_assemblers)
  h2a_call* d_calls = nullptr;  // their call blocks
  h2fc_link* d_fctab = nullptr;     // the links with a ledger, in spec order (grdma_h2_group_pipe_attach_flow_control)
  h2fc_call* d_fc_calls = nullptr;  // their call blocks
};

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
    if (parser_of(i)->fc) return h2_group_refuse(nullptr, "h2 group pipe: a parser with a flow-control ledger (single transport only)");
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
    if (r->seq) return h2_group_refuse(nullptr, "h2 group reply pipe: a reply bound to a pipe already");
    // (the source of a reply pipe assembles in forward pipes: a standalone source is framed by grdma_h2_reply_frame)
    if (!r->src->attached) return h2_group_refuse(nullptr, "h2 group reply pipe: a source assembler that is not attached to a forward pipe");
  }
  uint32_t have[2] = {0, 0};
  if (grdma_job_hook_counts(job, have) != 0) return nullptr;
  if (have[0] || have[1]) return h2_group_refuse(nullptr, "h2 group pipe: the job already carries hooks (another pipe's)");
  grdma_h2_group_pipe* p = new grdma_h2_group_pipe();
  h2_step_seq& s = p->seq;
  p->links.resize(n);
  std::vector<grdma_h2_link_frame> ftab(n);
  std::vector<grdma_h2_link_deframe> dtab(n);
  std::vector<h2r_link> rtab(n);
  const uint64_t per = H2_EMIT_THREADS / 64;
  uint32_t frame_grid = 0;
  bool ok = h2_seq_create(&s, job) && hipMalloc((void**)&p->d_ftab, sizeof(grdma_h2_link_frame) * n) == hipSuccess &&
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
    if (grdma_job_link_view(job, link_of(i), &l.d_sges, &l.count, &l.d_slices, &l.dst, &s.job_stream) != 0 ||
        grdma_job_link_step_slices(job, link_of(i), &d_step, &slices_cap) != 0)
      return h2_group_refuse(p, "h2 group pipe: a link index out of range");
    s.parsers.push_back(parser_of(i));
    l.ev_cap = specs ? specs[i].events_cap : rspecs[i].events_cap;
    l.hdr_cap = 32 * (l.count + 64);
    ok = hipMalloc((void**)&l.d_hdr, l.hdr_cap) == hipSuccess &&
         hipMalloc((void**)&l.d_ev, sizeof(grdma_h2_event) * (l.ev_cap ? l.ev_cap : 1)) == hipSuccess &&
         (specs ? h2_upload_msgs(specs[i].msgs, specs[i].nmsgs, &l.d_msgs)
                : h2_seq_bind_reply(&s, rspecs[i].reply, l.d_sges, l.count, l.d_hdr, l.hdr_cap, rspecs[i].recorded_wire_bytes));
    if (rspecs) rtab[i].R = rspecs[i].reply->d;
    const uint64_t nmsgs = specs ? specs[i].nmsgs : 0;
    grdma_h2_link_frame& f = ftab[i];
    f.msgs = l.d_msgs;
    f.nmsgs = nmsgs;
    f.out = l.d_sges;
    f.cap = l.count;
    f.hdr = l.d_hdr;
    f.hdr_cap = l.hdr_cap;
    f.res = p->d_fres + i;
    f.max_frame = max_frame;
    f.wg0 = frame_grid;
    frame_grid += (uint32_t)((nmsgs + per - 1) / per);
    // the step's own slice count, as the job's drain leaves it on the device (the recorded run's count is what the
    // caller expects; a step at another ring phase may deliver a slice more or less), bounded by the table
    grdma_h2_link_deframe& q = dtab[i];
    q.res = p->d_dres + i;
    q.gp = parser_of(i)->d;
    q.arena = l.dst;
    q.slices = l.d_slices;
    q.nslices = slices_cap;
    q.ev = l.d_ev;
    q.ev_cap = l.ev_cap;
    q.n_step = d_step;
  }
  s.deframe_stream = s.job_stream;  // (csrc: why the single pipe does the same by default)
  ok = ok && hipMemcpy(p->d_ftab, ftab.data(), sizeof(grdma_h2_link_frame) * n, hipMemcpyHostToDevice) == hipSuccess &&
       (!rspecs || hipMemcpy(p->d_rtab, rtab.data(), sizeof(h2r_link) * n, hipMemcpyHostToDevice) == hipSuccess) &&
       hipMemcpy(p->d_dtab, dtab.data(), sizeof(grdma_h2_link_deframe) * n, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    grdma_h2_group_pipe_destroy(p);
    grdma_fail_msg(GRDMA_ERR_HIP, "h2 group pipe: device allocation failed");
    return nullptr;
  }
  if (!h2_seq_install(&s, rspecs ? h2_stage_reply_links(p->d_rtab, n) : h2_stage_frame_links(p->d_ftab, n, frame_grid),
                      h2_stage_deframe_links(p->d_dtab, n))) {
    grdma_h2_group_pipe_destroy(p);
    return nullptr;
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

void grdma_h2_group_pipe_destroy(grdma_h2_group_pipe* p) {
  if (!p || h2_seq_read_by_reply_pipes(&p->seq)) return;
  h2_seq_destroy(&p->seq);
  for (h2_group_link& l : p->links) {
    hipFree(l.d_msgs);
    hipFree(l.d_hdr);
    hipFree(l.d_ev);
    hipFree(l.d_wu);
    hipFree(l.d_wu_hdr);
  }
  hipFree(p->d_fctab);
  hipFree(p->d_fc_calls);
  hipFree(p->d_rtab);
  hipFree(p->d_atab);
  hipFree(p->d_calls);
  hipFree(p->d_ftab);
  hipFree(p->d_dtab);
  hipFree(p->d_fres);
  hipFree(p->d_dres);
  delete p;
}

int grdma_h2_group_pipe_enqueue(grdma_h2_group_pipe* p) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p) return -GRDMA_ERR_INVALID;
  return h2_seq_enqueue(&p->seq, p->d_fres, sizeof(grdma_h2_frame_result) * p->links.size());
}

// Wait for the last step and report it: 14 words per listed link (h2_step_report; the stage times are the batch's,
// repeated)
int grdma_h2_group_pipe_sync(grdma_h2_group_pipe* p, uint64_t* out, uint64_t out_words) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !out || out_words < 14 * p->links.size()) return -GRDMA_ERR_INVALID;
  if (int rc = h2_seq_wait(&p->seq)) return rc;
  const size_t n = p->links.size();
  std::vector<grdma_h2_frame_result> fr(n);
  std::vector<grdma_h2_deframe_result> dr(n);
  if (hipMemcpy(fr.data(), p->d_fres, sizeof(grdma_h2_frame_result) * n, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(dr.data(), p->d_dres, sizeof(grdma_h2_deframe_result) * n, hipMemcpyDeviceToHost) != hipSuccess)
    return -GRDMA_ERR_HIP;
  for (size_t i = 0; i < p->seq.replies.size(); i++)  // (a link's overflow 2: its step had another shape than the recorded one)
    if (!h2_reply_result(p->seq.replies[i], &fr[i])) return -GRDMA_ERR_HIP;
  uint64_t f_us, d_us;
  h2_seq_stage_us(&p->seq, &f_us, &d_us);
  for (size_t i = 0; i < n; i++) h2_step_report(out + 14 * i, fr[i], dr[i], f_us, d_us);
  return 0;
}

int64_t grdma_h2_group_pipe_events(grdma_h2_group_pipe* p, uint32_t i, grdma_h2_event* out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || i >= p->links.size() || (!out && cap)) return -GRDMA_ERR_INVALID;
  if (int rc = h2_seq_wait(&p->seq)) return rc;
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
  if (int rc = h2_seq_wait(&p->seq)) return rc;
  if (l.count && hipMemcpy(out, l.d_sges, sizeof(grdma_sge) * l.count, hipMemcpyDeviceToHost) != hipSuccess) return -GRDMA_ERR_HIP;
  return (int64_t)l.count;
}

int grdma_h2_group_pipe_attach_assemblers(grdma_h2_group_pipe* p, grdma_h2_asm* const* asms, uint32_t n) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !asms) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: a pipe and an assembler list");
  if (n != p->links.size()) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: one assembler entry per link spec");
  if (!p->seq.asms.empty()) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: assemblers are attached already");
  uint32_t have = 0;
  for (uint32_t i = 0; i < n; i++) {
    grdma_h2_asm* a = asms[i];
    if (!a) continue;
    if (a->parser != p->seq.parsers[i]) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: an assembler of another parser than its link's");
    if (a->attached || a->parser->asm_attached) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: an assembler attached already");
    for (uint32_t k = 0; k < i; k++)
      if (asms[k] == a) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: the same assembler twice");
    have++;
  }
  if (!have) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: no assembler in the list");
  if (p->seq.launched && h2_seq_wait(&p->seq) != 0) return -GRDMA_ERR_HIP;
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
  return h2_seq_attach(&p->seq, h2_stage_asm_links(p->d_atab, have), asms, n);
}

int64_t grdma_h2_group_pipe_messages(grdma_h2_group_pipe* p, uint32_t i, grdma_h2_rx_msg* out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || i >= p->seq.asms.size() || !p->seq.asms[i] || (!out && cap)) return -GRDMA_ERR_INVALID;
  return h2_seq_messages(&p->seq, p->seq.asms[i], out, cap);
}

// The window ledgers' stage for the links listed with one: five kernels (k_h2_links_fc_*) however many links, behind what
// the pipe runs behind its job at the time of the call -- behind the assemblers' six if those were attached first, in
// front of them otherwise (the ledgers read the events only, so either order gives the same bytes).  The pipe owns each
// listed link's window-update list (room for that ledger's max_updates frames) and call block.  The create calls refuse
// a parser that has a ledger, so a ledger joins a group pipe by being created on its link's parser AFTER the pipe, then
// attached.  Ordering stays in h2_seq_enqueue: the stage adds no rule.
int grdma_h2_group_pipe_attach_flow_control(grdma_h2_group_pipe* p, grdma_h2_fc* const* fcs, uint32_t n) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || !fcs) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: a pipe and a ledger list");
  if (!p->seq.replies.empty()) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: a group reply pipe carries no window ledgers (not built)");
  if (n != p->links.size()) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: one ledger entry per link spec");
  if (!p->seq.fcs.empty()) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: ledgers are attached already");
  uint32_t have = 0;
  for (uint32_t i = 0; i < n; i++) {
    grdma_h2_fc* f = fcs[i];
    if (!f) continue;
    for (uint32_t k = 0; k < i; k++)
      if (fcs[k] == f) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: the same ledger twice");
    if (f->seq) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: a ledger attached to a pipe already");
    if (!f->parser) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: a ledger whose parser is gone");
    if (f->parser != p->seq.parsers[i]) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: the ledger of another parser than its link's");
    have++;
  }
  if (!have) return grdma_fail_msg(GRDMA_ERR_INVALID, "h2 group pipe: no ledger in the list");
  h2_host_ctx* hc = h2_ctx();
  if (!hc || hipStreamSynchronize(hc->stream) != hipSuccess) return -GRDMA_ERR_HIP;  // (the ledgers' standalone calls)
  if (p->seq.launched && h2_seq_wait(&p->seq) != 0) return -GRDMA_ERR_HIP;
  if ((!p->d_fctab && hipMalloc((void**)&p->d_fctab, sizeof(h2fc_link) * n) != hipSuccess) ||
      (!p->d_fc_calls && hipMalloc((void**)&p->d_fc_calls, sizeof(h2fc_call) * n) != hipSuccess))
    return -GRDMA_ERR_HIP;
  std::vector<h2fc_call> calls;
  std::vector<h2fc_link> tab;
  for (uint32_t i = 0; i < n; i++) {
    grdma_h2_fc* f = fcs[i];
    if (!f) continue;
    h2_group_link& l = p->links[i];
    if (!h2_fc_prepare(f, l.ev_cap)) return -GRDMA_ERR_HIP;
    l.wu_cap = (f->h.max_updates * H2FC_FRAME + H2_INLINED - 1) / H2_INLINED;
    if ((!l.d_wu && hipMalloc((void**)&l.d_wu, sizeof(grdma_sge) * l.wu_cap) != hipSuccess) ||
        (!l.d_wu_hdr && hipMalloc((void**)&l.d_wu_hdr, 32 * l.wu_cap) != hipSuccess) ||
        !h2_fc_set_target(f, l.d_wu, l.wu_cap, l.d_wu_hdr, 32 * l.wu_cap, nullptr))
      return -GRDMA_ERR_HIP;
    tab.push_back(h2fc_link{f->d, p->d_fc_calls + calls.size()});
    calls.push_back(h2fc_call{l.d_ev, p->d_dres + i, l.ev_cap});
  }
  if (hipMemcpy(p->d_fc_calls, calls.data(), sizeof(h2fc_call) * have, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(p->d_fctab, tab.data(), sizeof(h2fc_link) * have, hipMemcpyHostToDevice) != hipSuccess)
    return -GRDMA_ERR_HIP;
  if (int rc = h2_seq_append(&p->seq, h2_stage_fc_links(p->d_fctab, have))) return rc;
  p->seq.fcs.assign(fcs, fcs + n);
  for (grdma_h2_fc* f : p->seq.fcs)
    if (f) f->seq = &p->seq;
  return 0;
}

int64_t grdma_h2_group_pipe_window_updates(grdma_h2_group_pipe* p, uint32_t i, grdma_slice* slices_out, uint64_t cap, uint64_t out[8]) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || i >= p->seq.fcs.size() || !p->seq.fcs[i] || !out || (!slices_out && cap)) return -GRDMA_ERR_INVALID;
  return h2_seq_window_updates(&p->seq, p->seq.fcs[i], p->links[i].d_wu, slices_out, cap, out);
}

int64_t grdma_h2_group_pipe_window_update_bytes(grdma_h2_group_pipe* p, uint32_t i, void* bytes_out, uint64_t cap) {
  if (grdma_device_count() <= 0) return -GRDMA_ERR_NO_DEVICE;
  if (!p || i >= p->seq.fcs.size() || !p->seq.fcs[i] || (!bytes_out && cap)) return -GRDMA_ERR_INVALID;
  return h2_seq_window_update_bytes(&p->seq, p->seq.fcs[i], p->links[i].d_wu_hdr, bytes_out, cap);
}
