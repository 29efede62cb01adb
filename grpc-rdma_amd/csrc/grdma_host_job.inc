// The device-resident streaming job: links, the C ABI of grdma_stream_job_*, and the schedule of a job's rounds.  The
// schedule is stated ONCE: job_stage_launch (what a stage launches) and job_schedule (sequential / paired / limit-driven:
// the steps and what each waits for); job_build_graph, job_enqueue_chain and job_enqueue_streams only emit it.
// (part of the host layer: textually included by grdma_pair.hip -- one translation unit, so that the pair
//  structure and the helpers in its unnamed namespaces stay internal)
// ---- device-resident streaming job -------------------------------------------------
// n independent links (connections) advance in lock step: every launch carries one
// op per link (grid.y = n), so 32 connections with 4 MiB rings fill the chip the way
// one connection with a 128 MiB ring would.
struct grdma_job_link {
  grdma_pair* tx = nullptr;
  grdma_pair* rx = nullptr;
  grdma_sge* d_sges = nullptr;
  uint64_t count = 0;
  grdma_slice_out* d_slices = nullptr;
  uint64_t slices_cap = 0;
  uint8_t* dst = nullptr;
  uint64_t dst_cap = 0;
  // second copies of what two rounds in flight would otherwise share (pipelined mode)
  // index of the slice buffer (k_tx_index / k_tx_fast, grdma_tx_fast.hip): [count + 1] entries each
  uint64_t* d_encpre = nullptr;
  uint64_t* d_lenpre = nullptr;
  uint32_t* d_tilepre = nullptr;
  grdma_plan* d_wireplan2 = nullptr;
  grdma_plan* d_rxplan2 = nullptr;
  uint8_t* d_staging2 = nullptr;
  uint8_t* d_staging_n[2] = {nullptr, nullptr};  // grdma_stream_job_set_sends: both parities' staging for several Sends per plan
};

struct grdma_stream_job {
  std::vector<grdma_job_link> links;
  uint64_t rounds = 0;
  // device control block: txop[3][n], rxop[3][n], results, plan pointer arrays.
  // Op set 0 is the first round (resets the cursors), sets 1 / 2 are odd / even rounds:
  // they differ in which of the doubled buffers (wire plan, staging, scatter plan,
  // drain result) they use, so that two rounds can be in flight.
  uint8_t* d_ctl = nullptr;
  grdma_tx_op* d_txop = nullptr;      // [3 * n]
  grdma_rx_op* d_rxop = nullptr;      // [3 * n]
  grdma_tx_result* d_txres = nullptr; // [n]
  grdma_rx_result* d_rxres = nullptr; // [2 * n]
  const grdma_plan** d_plans = nullptr;  // [3 * n]: gather, wire (even), wire (odd)
  grdma_size_hint* d_hints = nullptr; // [3 * n]: the record sizes the Send of a round computed, per op set: what the
                                      // drain of the same round predicts the ring's records from (grdma_rx_op::sizes_in)
  uint64_t* d_limits = nullptr;       // [3 * n]: remote_tail_ after the Send(s) of a round, per op set: what the
                                      // drain of the same round may walk up to (grdma_rx_op::limit_ptr)
  grdma_conn** d_txconns = nullptr;   // [n]: the sending ends, for the arrival report behind the last round
  hipGraphExec_t exec = nullptr;
  // kernel nodes another stage hangs in front of / behind the job inside its graph (grdma_job_set_hooks: the HTTP/2
  // pipe's framing and deframing): a chain in front of the first round, a chain behind k_tx_commit
  std::vector<grdma_job_hook> pre_hooks, post_hooks;
  uint64_t hooks_gen = 0, exec_hooks_gen = 0;
  uint64_t exec_rounds = 0;
  int exec_pipeline = -1;
  int exec_fastkey = -1;              // job_fastkey of the job the graph was built for (planner kernels, Sends per plan, modes)
  int runs = 0;
  int rx_miss = 0, tx_miss = 0;       // consecutive runs whose drains / Sends of link 0 mostly went to the general planner
  uint64_t seen[4] = {0, 0, 0, 0};    // the result blocks' taken / declined counters at the end of the last run
  int pipeline = 0;                   // 1: overlap the send plan / gather / scatter of
                                      // neighbouring rounds on side streams
  hipStream_t s_wire = nullptr, s_rxplan = nullptr, s_apply = nullptr;
  int tx_fast = 1;                    // Sends of one-Send rounds are priced from an index of the slice buffer: k_tx_index at
                                      // the start of a step, k_tx_fast per Send, the general planner behind it for the rest
                                      // (0: the general planner alone -- grdma_stream_job_run, after repeated declines)
  grdma_txf_ctl* d_txf = nullptr;     // [n]
  int fuse_wire = 1;                  // paired schedule, few links with small rings: the wire of round t inside the planner
                                      // pair's launch (k_plan_pair_mw's wire workgroups) -- two launches per round;
                                      // grdma_stream_job_set_fused_wire(j, 0): a k_copy launch of its own, as for every other job
  // The index of the slice table (k_tx_index) is a function of the table alone, and the job owns the table: built by
  // the first run, kept for the later ones -- unless something may rewrite the table between steps (kernel nodes hung
  // in front of the job, or a caller that asked where the table lives: the HTTP/2 pipe does both).
  bool index_valid = false, sges_exposed = false;
  int promise = 0;                    // grdma_stream_job_set_promised_credit: the Send of round t + 1 waits, inside the planner
                                      // pair's launch, for the drain plan of round t and is priced with the credit that
                                      // drain's scatter will post (k_plan_pair_mw) -- the paired schedule without its round
                                      // of credit lag
  uint32_t sends = 1;                 // grdma_stream_job_set_sends: consecutive Sends one round's plan holds (paired schedule,
                                      // planners of grdma_tx_multi.h / grdma_rx_multi.h: 16 workgroups per Send's worth of records)
  int rx_fast = 1;                    // drains of one-Send rounds go through k_rx_fast first (grdma_rx_fast.hip), the
                                      // general planner behind it only does what that kernel declined
                                      // (0: the general planner alone -- grdma_stream_job_run, after repeated declines)
  std::vector<hipEvent_t> pev;        // dependency events of the streams emitter (job_enqueue_streams)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> kev;
  std::vector<int> kev_cls;                   // timed passes: the class of the launch between marks i and i + 1
  hipStream_t stream = nullptr;
  bool direct = false;
  uint64_t max_ring = 0;
};

namespace {

inline int job_opset(uint64_t round) { return round == 0 ? 0 : ((round & 1) ? 1 : 2); }
inline bool job_index_needed(const grdma_stream_job* j) { return !j->index_valid || !j->pre_hooks.empty() || j->sges_exposed; }
inline int job_fastkey(const grdma_stream_job* j) {
  return (j->rx_fast ? 1 : 0) | (j->tx_fast ? 2 : 0) | (j->fuse_wire ? 128 : 0) | ((int)(j->sends & 7) << 8) |
         (job_index_needed(j) ? (1 << 12) : 0) | (j->promise ? (1 << 13) : 0) | ((int)j->sends << 16);
}
inline bool job_exec_stale(const grdma_stream_job* j) {
  return !j->exec || j->exec_rounds != j->rounds || j->exec_pipeline != j->pipeline || j->exec_fastkey != job_fastkey(j) ||
         j->exec_hooks_gen != j->hooks_gen;
}
// copy-kernel workgroups per link for `bytes` (gather and wire: half a ring, scatter: a ring), the grid of all links kept
// around 2048 workgroups in total
inline uint32_t job_copy_blocks(const grdma_stream_job* j, uint64_t bytes) {
  const uint32_t grid_cap = copy_blocks_for(~0ull >> 8);
  return std::max<uint32_t>(1, std::min<uint32_t>(copy_blocks_for(bytes), grid_cap / (uint32_t)j->links.size() + 1));
}
// The parameters of a job kernel launched by address (hipLaunchKernel, a graph's kernel node): three pointers, the
// planner pair's 4-byte workgroup split and its wire plans, padded to GRDMA_JOB_HOOK_ARGS entries -- the runtime reads as
// many as the kernel has, a kernel with fewer ignores the rest.  `v` points into the object: keep it alive for the call.
struct job_kargs {
  const void* p[3];
  uint32_t split;
  const void* wire;
  void* v[GRDMA_JOB_HOOK_ARGS];
  job_kargs(const void* a0, const void* a1, const void* a2, uint32_t a3 = 0, const void* a4 = nullptr)
      : p{a0, a1, a2}, split(a3), wire(a4) {
    static uint64_t none = 0;
    for (void*& x : v) x = &none;
    v[0] = &p[0]; v[1] = &p[1]; v[2] = &p[2]; v[3] = &split; v[4] = &wire;
  }
  job_kargs(const job_kargs&) = delete;
  job_kargs& operator=(const job_kargs&) = delete;
};

// planner workgroups of a round: sixteen per Send's worth of records
// (up to two Sends: priced one after the other, each may carry 4095 records.  More: folded into one cut of the index,
//  a round carries at most sends x max_sge records -- 256 of them per workgroup)
inline uint32_t job_groups(const grdma_stream_job* j, uint32_t per_send) {
  // (round 6) ... and never more than the job's slice tables can fill: a round carries at most one record per slice of
  // the table plus one per Send (a slice cut by the free space goes out as two records), so a link of a few hundred
  // slices -- 32 connections x 64 KiB messages -- is planned by 3 + 3 workgroups instead of 16 + 16: a launch of 192
  // planner workgroups for 32 links where there were 1024, every one of them resident at once.  A drain that finds more
  // records than its workgroups cover declines, and the general planner walks it: slower, never wrong.
  uint64_t slices = 1;
  for (const grdma_job_link& l : j->links) slices = std::max<uint64_t>(slices, l.count);
  const bool seq_sends = j->sends <= grdma_tx_multi_seq_sends();
  const uint64_t by_table = ((slices + j->sends + 1 + 255) / 256) * (seq_sends ? j->sends : 1);
  uint64_t g;
  if (seq_sends) {
    g = (uint64_t)per_send * j->sends;
  } else {
    uint64_t most = 1;
    for (const grdma_job_link& l : j->links) most = std::max<uint64_t>(most, (uint64_t)j->sends * l.tx->max_sge);
    g = std::min<uint64_t>(2 * per_send, (most + 255) / 256);
  }
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(g, by_table));
}
inline uint32_t job_rx_groups(const grdma_stream_job* j) { return job_groups(j, grdma_rx_multi_groups()); }
inline uint32_t job_tx_groups(const grdma_stream_job* j) { return job_groups(j, grdma_tx_multi_groups()); }
inline bool job_mw(const grdma_stream_job* j) { return j->pipeline && j->rx_fast && j->tx_fast; }
// the sequential schedule (five launches per round, strictly in order) with the small planner workgroups: what carries
// several Sends per plan when the job is not pipelined -- a ring every round fills sees its credit at once here, a round
// late on the paired schedule
inline bool job_mw_seq(const grdma_stream_job* j) { return j->sends > 1 && !j->pipeline && j->rx_fast && j->tx_fast; }
// compute units of the current device (0: unknown)
inline int job_device_cus() {
  static const int cus = [] {
    int dev = 0, c = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c = 0;
    return c;
  }();
  return cus;
}
// Promised credit (k_plan_pair_mw): the Send's workgroups of the planner pair's launch wait for the drain plan of the same
// launch.  The invariant that keeps this wait, and every other wait between the workgroups of a job's launch, from
// deadlocking (stated here once): workgroups are dispatched in index order, x (the link) fastest, then y; a workgroup
// waits only on workgroups with a LOWER blockIdx (wire, then drain, then Send workgroups; a committer is the last of its
// group); and every wait is bounded -- one that runs out is given up (the promise: csrc/grdma_devfn.h, the wire:
// csrc/grdma_rx_multi.h).  So whatever a workgroup waits for has a CU or is done before it gets one, and no planner
// workgroup needs to be resident beside the others.  Through the first half of round 6 the mode also required that
// (links x (G + H) <= CUs); GRDMA_JOB_PROMISE_RESIDENT=1 restores the condition -- the fallback should a runtime ever
// dispatch out of order.  64 links of BASELINE configs[3] at 3 + 3 workgroups are 384: the steady state of that leg is
// 373 -> 440 GiB/s without it.
inline bool job_promise(const grdma_stream_job* j) {
  // (staged wire only: with a direct wire the gather of round t + 1 writes the ring in the launch of round t's scatter)
  if (!j->promise || !job_mw(j) || j->direct) return false;
  static const bool resident_only = getenv("GRDMA_JOB_PROMISE_RESIDENT") && atoi(getenv("GRDMA_JOB_PROMISE_RESIDENT")) != 0;
  if (!resident_only) return true;
  return (uint64_t)j->links.size() * (job_rx_groups(j) + job_tx_groups(j)) <= (uint64_t)job_device_cus();
}
// Wire workgroups of the planner pair's launch (0: the wire is a k_copy launch of its own).  The planner kernel runs one
// workgroup per CU (its LDS), a wave of it moves one tile at a time: only a round of a few MiB is moved as fast by W of
// them as by k_copy's grid, and the drain's workgroups WAIT for the wire's inside the launch -- so, for speed, every
// workgroup of the launch must have a CU at once (what makes the wait safe is job_promise's invariant).  One per four
// 8 KiB tiles of half a ring, at least 8, at most 64.
inline uint32_t job_wire_groups(const grdma_stream_job* j) {
  if (!j->fuse_wire || !job_mw(j) || j->direct || j->max_ring > (16ull << 20)) return 0;
  const uint32_t w = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(8, (j->max_ring / 2 / 8192 + 3) / 4));
#ifdef GRDMA_WAVE_EMU
  return w;  // (the emulator runs the workgroups of a launch one after the other, in index order: the wire's first)
#else
  return (uint64_t)j->links.size() * (w + job_rx_groups(j) + job_tx_groups(j)) <= (uint64_t)job_device_cus() ? w : 0;
#endif
}
inline uint32_t job_pair_mode(const grdma_stream_job* j) {
  return job_rx_groups(j) | (job_promise(j) ? (1u << 16) : 0u) | (job_wire_groups(j) << 20);
}
inline uint32_t job_index_blocks(const grdma_stream_job* j) {  // k_tx_index: 1024 slices per workgroup
  uint64_t most = 1;
  for (const grdma_job_link& l : j->links) most = std::max<uint64_t>(most, l.count);
  return (uint32_t)((most + 1023) / 1024);
}
// ---- the schedule of a job, stated once ---------------------------------------------------------------------------
// job_stage_launch says WHAT a stage of a round launches (kernel, grid, the five job_kargs values), job_schedule says IN
// WHAT ORDER: the steps of a schedule in creation order, each with the steps it waits for.  The three emitters behind
// them (a HIP graph, a chain on one stream, the streams) only walk that list -- docs/job_planners.md, "The host side".
enum job_stage {
  JOB_INDEX,           // k_tx_index in front of round 0: the index of the slice table the Sends are priced from
  JOB_SEND_PLAN,       // P_t
  JOB_GATHER,          // G_t
  JOB_WIRE,            // W_t
  JOB_DRAIN_PLAN,      // X_t
  JOB_SCATTER,         // A_t
  JOB_PAIR,            // X_t + P_{t+1} in one launch (k_plan_pair_mw), with or without the wire's workgroups
  JOB_SCATTER_GATHER,  // A_t + G_{t+1} in one launch (k_rx_apply_gather)
  JOB_COMMIT           // behind the last round: the connection's arrival report and the state lines (k_tx_commit)
};
enum job_schedule_kind { JOB_SEQUENTIAL, JOB_PAIRED, JOB_LIMIT_DRIVEN };
// One launch.  fn == nullptr: the stage does not exist in this round (the wire of a direct wire, a wire the planner
// pair's launch carries, an index that is kept).  cls is the time class of grdma_stream_result::ms_class; -1 = none: a
// timed pass records no event behind it, so the index counts towards the send plan it precedes.
struct job_launch {
  int cls = -1;
  const void* fn = nullptr;
  dim3 grid;
  uint32_t threads = 0;
  const void *a0 = nullptr, *a1 = nullptr, *a2 = nullptr;
  uint32_t split = 0;
  const void* wire = nullptr;
};
// `as_graph`: the launches of a job's GRAPH (and of the timed chain that mirrors it) rather than of an eager pass.
job_launch job_stage_launch(const grdma_stream_job* j, job_schedule_kind kind, bool as_graph, job_stage stage, uint64_t t) {
  const uint32_t n = (uint32_t)j->links.size();
  const uint32_t txb = job_copy_blocks(j, j->max_ring / 2), rxb = job_copy_blocks(j, j->max_ring);
  const uint32_t pt = grdma_kernel_threads(0), ct = grdma_kernel_threads(1);
  const void* txop = j->d_txop + job_opset(t) * n;
  const void* rxop = j->d_rxop + job_opset(t) * n;
  const void* gplans = j->d_plans;
  const void* wplans = j->d_plans + n * (1 + (t & 1));
  // several Sends per plan: only the planners of grdma_tx_multi.h / grdma_rx_multi.h handle those -- k_plan_pair_mw with
  // the workgroups of one side alone (job_mw_seq: the sequential schedule; job_mw: the eager passes of a paired job)
  const bool multi = j->sends > 1 && (job_mw(j) || job_mw_seq(j));
  // few links with small rings: the wire rides in the planner pair's launch (the paired schedule only)
  const uint32_t wg_wire = kind == JOB_PAIRED ? job_wire_groups(j) : 0;
  auto make = [](int cls, const void* fn, dim3 grid, uint32_t threads, const void* a0, const void* a1 = nullptr,
                 const void* a2 = nullptr, uint32_t split = 0, const void* wire = nullptr) {
    job_launch l;
    l.cls = cls; l.fn = fn; l.grid = grid; l.threads = threads;
    l.a0 = a0; l.a1 = a1; l.a2 = a2; l.split = split; l.wire = wire;
    return l;
  };
  switch (stage) {
    case JOB_INDEX:  // (once per job unless the table may change between steps; only Sends priced from it need it)
      if (t != 0 || !j->tx_fast || !job_index_needed(j)) return job_launch();
      return make(-1, grdma_kernel_fn_tx_index(), dim3(job_index_blocks(j), n), grdma_tx_index_threads(), j->d_txf);
    case JOB_SEND_PLAN: {
      if (!j->tx_fast) return make(0, grdma_kernel_fn(0), dim3(n), pt, txop);
      // ODDITY (kept): the first Send of a pipelined job's graph is priced by the planner pair's Send workgroups
      // (k_plan_pair_mw with no drain); the eager passes give round 0 to k_tx_plan_job like every other round
      const bool first_send_of_graph = as_graph && t == 0 && (j->pipeline || job_mw_seq(j));
      if (first_send_of_graph || multi)
        return make(0, grdma_kernel_fn_plan_pair_mw(), dim3(n, job_tx_groups(j)), pt, nullptr, txop, j->d_txf, 0u);
      // priced from the index, the general planner behind it in the same launch for what that declines
      return make(0, grdma_kernel_fn(6), dim3(n), grdma_tx_plan_job_threads(), txop, j->d_txf);
    }
    case JOB_GATHER:
      return make(1, grdma_kernel_fn(1), dim3(txb, n), ct, gplans);
    case JOB_WIRE:  // (a direct wire has no wire kernel: the gather writes the records into the peer ring)
      if (j->direct || wg_wire) return job_launch();
      return make(2, grdma_kernel_fn(1), dim3(txb, n), ct, wplans);
    case JOB_DRAIN_PLAN:
      // ODDITY (kept): the drain's planners alone get job_rx_groups as the split word, the Send's alone get 0
      if (multi) return make(3, grdma_kernel_fn_plan_pair_mw(), dim3(n, job_rx_groups(j)), pt, rxop, nullptr, j->d_txf, job_rx_groups(j));
      // k_rx_plan_job = the straight-line steady-state body, then the general planner for what it declines
      if (j->rx_fast) return make(3, grdma_kernel_fn_rx_plan_job(), dim3(n), grdma_rx_plan_job_threads(), rxop);
      return make(3, grdma_kernel_fn_rx_plan(), dim3(n), pt, rxop);
    case JOB_SCATTER:
      return make(4, grdma_kernel_fn(3), dim3(rxb, n), ct, rxop);
    case JOB_PAIR: {  // the drain of round t and the Send of round t + 1 (none behind the last round)
      const bool more = t + 1 < j->rounds;
      return make(5, grdma_kernel_fn_plan_pair_mw(), dim3(n, wg_wire + job_rx_groups(j) + (more ? job_tx_groups(j) : 0)), pt, rxop,
                  more ? j->d_txop + job_opset(t + 1) * n : nullptr, j->d_txf, job_pair_mode(j), wg_wire ? wplans : nullptr);
    }
    case JOB_SCATTER_GATHER:  // (both are ready behind the planner pair, neither touches the other's bytes)
      return make(6, grdma_kernel_fn(8), dim3(std::max(rxb, txb), 2 * n), ct, rxop, gplans);
    case JOB_COMMIT:
      return make(-1, grdma_kernel_fn(5), dim3(n), 64, j->d_txconns);
  }
  return job_launch();
}
hipError_t job_launch_on(const job_launch& l, hipStream_t s) {
  job_kargs a(l.a0, l.a1, l.a2, l.split, l.wire);
  return hipLaunchKernel(l.fn, l.grid, dim3(l.threads), a.v, 0, s);
}

// A step of a schedule: a launch and the EARLIER steps (indices into the list) it waits for.
struct job_step {
  job_stage stage;
  job_launch l;
  std::vector<int> deps;
};
// The three schedules (t = round; P send plan, G gather, W wire, X drain plan, A scatter; W|G = the wire, or the gather
// where the round has no wire launch).  Steps come in creation order -- per round P G W X A -- and absent stages are left
// out, so every emitter sees only what is launched.
//   sequential     P_t <- A_{t-1}    G_t <- P_t    W_t <- G_t    X_t <- (W|G)_t    A_t <- X_t
//   paired         kernels of different branches of a graph do not overlap on this stack (measured), so the round is a
//                  chain: [index] P_0 G_0, then per round W_t <- G_t, the planner pair X_t + P_{t+1} <- (W|G)_t, A_{t-1},
//                  and A_t + G_{t+1} <- X_t (the plain scatter behind the last round): three launches per round, two
//                  where the pair's launch carries the wire
//   limit-driven   a pipelined job on the general planners.  The drain of round t walks exactly up to the tail its Send
//                  computed (grdma_rx_op::limit_ptr), so round t + 1 may land in the ring while round t is walked:
//                    P_t <- P_{t-1} (the sender's state), G_{t-1} (one gather plan), (W|G)_{t-2} (staging / wire plan
//                           of this parity), A_{t-2} (credit lag of at most one round; implies X_{t-2}: the limit slot)
//                    G_t <- P_t        W_t <- G_t
//                    X_t <- (W|G)_t, X_{t-1} (the reader's state), A_{t-2} (scatter plan / result of this parity)
//                    A_t <- X_t, A_{t-1} (credit reports stay in order)
//                  the only cycle that spans rounds is A_{t-2} -> P_t -> G_t -> W_t -> X_t -> A_t: two rounds in flight
//   all three      index <- nothing, P_0 <- index;    commit <- (W|G)_{R-1}, A_{R-1}
// The sender may see the credit of a scatter a round later than on the sequential schedule; with rounds of at most
// ring / 6 that never limits a Send.
std::vector<job_step> job_schedule(const grdma_stream_job* j, job_schedule_kind kind, bool as_graph) {
  const uint64_t R = j->rounds;
  std::vector<job_step> steps;
  std::vector<int> P(R, -1), G(R, -1), W(R, -1), X(R, -1), A(R, -1);  // the step that holds a stage of round t
  auto add = [&](job_stage stage, uint64_t t, std::initializer_list<int> deps) -> int {
    job_step s{stage, job_stage_launch(j, kind, as_graph, stage, t), {}};
    if (!s.l.fn) return -1;
    for (int d : deps)
      if (d >= 0 && std::find(s.deps.begin(), s.deps.end(), d) == s.deps.end()) s.deps.push_back(d);  // (a node twice is an invalid argument)
    steps.push_back(s);
    return (int)steps.size() - 1;
  };
  auto at = [](const std::vector<int>& v, uint64_t t, uint64_t back) { return t >= back ? v[t - back] : -1; };
  auto wire_at = [&](uint64_t t, uint64_t back) { return at(W, t, back) >= 0 ? at(W, t, back) : at(G, t, back); };
  for (uint64_t t = 0; t < R; t++) {
    const int index = t == 0 ? add(JOB_INDEX, 0, {}) : -1;
    switch (kind) {
      case JOB_SEQUENTIAL:
        P[t] = add(JOB_SEND_PLAN, t, {index, at(A, t, 1)});
        G[t] = add(JOB_GATHER, t, {P[t]});
        W[t] = add(JOB_WIRE, t, {G[t]});
        X[t] = add(JOB_DRAIN_PLAN, t, {wire_at(t, 0)});
        A[t] = add(JOB_SCATTER, t, {X[t]});
        break;
      case JOB_PAIRED:
        if (t == 0) {
          P[0] = add(JOB_SEND_PLAN, 0, {index});
          G[0] = add(JOB_GATHER, 0, {P[0]});
        }
        W[t] = add(JOB_WIRE, t, {G[t]});
        X[t] = add(JOB_PAIR, t, {wire_at(t, 0), at(A, t, 1)});
        if (t + 1 < R) {
          P[t + 1] = X[t];
          A[t] = G[t + 1] = add(JOB_SCATTER_GATHER, t, {X[t]});
        } else {
          A[t] = add(JOB_SCATTER, t, {X[t]});
        }
        break;
      case JOB_LIMIT_DRIVEN:
        P[t] = add(JOB_SEND_PLAN, t, {index, at(P, t, 1), at(G, t, 1), wire_at(t, 2), at(A, t, 2)});
        G[t] = add(JOB_GATHER, t, {P[t]});
        W[t] = add(JOB_WIRE, t, {G[t]});
        X[t] = add(JOB_DRAIN_PLAN, t, {wire_at(t, 0), at(X, t, 1), at(A, t, 2)});
        A[t] = add(JOB_SCATTER, t, {X[t], at(A, t, 1)});
        break;
    }
  }
  // the drains of the job were told how far to walk by their op (limit_ptr); the connection's own arrival report and
  // the state lines follow once, behind the last round.  ODDITY (kept): a job of no rounds has an empty graph, its
  // eager passes still launch the commit.
  if (R > 0) add(JOB_COMMIT, R - 1, {wire_at(R, 1), A[R - 1]});
  else if (!as_graph) add(JOB_COMMIT, 0, {});
  return steps;
}
// the schedule of a job's graph
inline job_schedule_kind job_graph_kind(const grdma_stream_job* j) {
  return !j->pipeline ? JOB_SEQUENTIAL : job_mw(j) ? JOB_PAIRED : JOB_LIMIT_DRIVEN;
}
// GRDMA_RUN_INSTRUMENTED_SCHEDULE times the graph's own chain; only the paired schedule is one
bool job_is_paired(const grdma_stream_job* j) { return job_mw(j) && j->rounds >= 1; }

// ---- emitter 1 of 3: a chain on one stream -------------------------------------------------------------------------
// The steps of a sequential or paired schedule one after the other (their creation order is their order).  `timed`: an
// event in front of the first launch and behind every launch with a class, the classes in kev_cls -- what
// grdma_stream_job_run turns into ms_class / launches_class.  GRDMA_RUN_INSTRUMENTED is the sequential chain (also of a
// pipelined job), GRDMA_RUN_INSTRUMENTED_SCHEDULE the paired one with the graph's launches: the same work in the same
// order as the graph, plus the time of each launch by itself.
int job_enqueue_chain(grdma_stream_job* j, job_schedule_kind kind, bool as_graph, hipStream_t s, bool timed) {
  size_t e = 0;
  auto mark = [&]() -> int {
    if (e >= j->kev.size()) {
      hipEvent_t ev;
      HIP_TRY(hipEventCreate(&ev));
      j->kev.push_back(ev);
    }
    HIP_TRY(hipEventRecord(j->kev[e++], s));
    return 0;
  };
  if (timed) {
    j->kev_cls.clear();
    if (int rc = mark()) return rc;
  }
  for (const job_step& st : job_schedule(j, kind, as_graph)) {
    HIP_TRY(job_launch_on(st.l, s));
    if (!timed || st.l.cls < 0) continue;
    if (int rc = mark()) return rc;
    j->kev_cls.push_back(st.l.cls);
  }
  return 0;
}

// ---- emitter 2 of 3: the limit-driven schedule as a software pipeline over four streams ---------------------------
// Every stage has a home stream (send plan, gather, index and commit: the job's own; wire, drain plan and scatter: a
// side stream each), a step waits for an event only where the step it depends on sits on another stream -- stream order
// gives the rest, and adds W_{t-1} -> W_t.  The waits in front of the commit are the join of the side streams.
int job_enqueue_streams(grdma_stream_job* j, hipStream_t s) {
  const std::vector<job_step> steps = job_schedule(j, JOB_LIMIT_DRIVEN, false);
  if (!j->s_wire) {
    HIP_TRY(hipStreamCreateWithFlags(&j->s_wire, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&j->s_rxplan, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&j->s_apply, hipStreamNonBlocking));
  }
  while (j->pev.size() < steps.size() + 1) {  // one per step (used where another stream waits for it) and the fork
    hipEvent_t ev;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    j->pev.push_back(ev);
  }
  auto home = [&](const job_step& st) {
    return st.stage == JOB_WIRE ? j->s_wire : st.stage == JOB_DRAIN_PLAN ? j->s_rxplan : st.stage == JOB_SCATTER ? j->s_apply : s;
  };
  std::vector<bool> watched(steps.size(), false);
  for (const job_step& st : steps)
    for (int d : st.deps)
      if (home(steps[d]) != home(st)) watched[d] = true;
  // the fork: the side streams start behind whatever the job's stream was given before
  hipEvent_t fork = j->pev[steps.size()];
  HIP_TRY(hipEventRecord(fork, s));
  if (!j->direct) HIP_TRY(hipStreamWaitEvent(j->s_wire, fork, 0));
  HIP_TRY(hipStreamWaitEvent(j->s_rxplan, fork, 0));
  HIP_TRY(hipStreamWaitEvent(j->s_apply, fork, 0));
  for (size_t i = 0; i < steps.size(); i++) {
    for (int d : steps[i].deps)
      if (home(steps[d]) != home(steps[i])) HIP_TRY(hipStreamWaitEvent(home(steps[i]), j->pev[d], 0));
    HIP_TRY(job_launch_on(steps[i].l, home(steps[i])));
    if (watched[i]) HIP_TRY(hipEventRecord(j->pev[i], home(steps[i])));
  }
  return 0;
}

// ---- emitter 3 of 3: the job as an explicitly built HIP graph -----------------------------------------------------
// One kernel node per step, its dependencies the nodes of the steps it waits for.  Built node by node rather than
// recorded from the streams: the dependency structure is known here, and it keeps the replay independent of how a
// runtime records cross-stream joins.  Nodes are added in the steps' order (a node's dependencies exist before it; the
// runtime may assign branches by that order).  The pre-hooks are a chain in front of the job's roots, the post-hooks a
// chain behind k_tx_commit, which every node of the job reaches.  Every node hands over GRDMA_JOB_HOOK_ARGS parameter
// slots (job_kargs); a kernel with fewer ignores the rest.
int job_build_graph(grdma_stream_job* j, hipGraph_t* out) {
  const std::vector<job_step> steps = job_schedule(j, job_graph_kind(j), true);
  hipGraph_t g;
  HIP_TRY(hipGraphCreate(&g, 0));
  hipError_t e = hipSuccess;
  auto add_node = [&](const void* fn, dim3 grid, uint32_t threads, void** params, const std::vector<hipGraphNode_t>& deps) -> hipGraphNode_t {
    hipKernelNodeParams np;
    memset(&np, 0, sizeof(np));
    np.func = const_cast<void*>(fn);
    np.gridDim = grid;
    np.blockDim = dim3(threads);
    np.kernelParams = params;
    hipGraphNode_t node = nullptr;
    if (e == hipSuccess) e = hipGraphAddKernelNode(&node, g, deps.empty() ? nullptr : deps.data(), deps.size(), &np);
    return node;
  };
  // hook nodes: a chain of kernels; `after` (may be null) is what the first one waits for, the last one is returned
  auto add_hooks = [&](std::vector<grdma_job_hook>& hooks, hipGraphNode_t after) -> hipGraphNode_t {
    for (grdma_job_hook& h : hooks) {
      void* args[GRDMA_JOB_HOOK_ARGS];
      for (uint32_t a = 0; a < GRDMA_JOB_HOOK_ARGS; a++) args[a] = &h.args[a];
      after = add_node(h.fn, dim3(h.grid), h.threads, args, after ? std::vector<hipGraphNode_t>{after} : std::vector<hipGraphNode_t>{});
    }
    return after;
  };
  std::vector<hipGraphNode_t> nodes(steps.size(), nullptr);
  if (!steps.empty()) {
    const hipGraphNode_t pre_last = add_hooks(j->pre_hooks, nullptr);
    for (size_t i = 0; i < steps.size() && e == hipSuccess; i++) {
      std::vector<hipGraphNode_t> deps;
      for (int d : steps[i].deps) deps.push_back(nodes[d]);
      if (deps.empty() && pre_last) deps.push_back(pre_last);  // a root of the job waits for the stage in front of it
      const job_launch& l = steps[i].l;
      job_kargs a(l.a0, l.a1, l.a2, l.split, l.wire);
      nodes[i] = add_node(l.fn, l.grid, l.threads, a.v, deps);
    }
    add_hooks(j->post_hooks, nodes.back());  // (the commit is the last step)
  }
  if (e != hipSuccess) {
    hipGraphDestroy(g);
    return fail(GRDMA_ERR_HIP, "graph construction failed: %s", hipGetErrorString(e));
  }
  *out = g;
  return 0;
}

}  // namespace

extern "C" {

grdma_stream_job* grdma_stream_job_create_multi(uint32_t n, grdma_pair* const* tx,
                                                grdma_pair* const* rx, const grdma_slice* slices,
                                                const uint64_t* counts, void* const* rx_dsts,
                                                const uint64_t* rx_dst_caps,
                                                const uint64_t* slices_caps, uint64_t max_rounds) {
  if (require_ctx()) return nullptr;
  if (!n || !tx || !rx || !slices || !counts || !rx_dsts || !rx_dst_caps || !slices_caps) {
    fail(GRDMA_ERR_INVALID, "stream job: null argument");
    return nullptr;
  }
  grdma_stream_job* j = new grdma_stream_job();
  j->rounds = max_rounds;
  j->stream = tx[0]->stream;
  j->direct = (tx[0]->flags & GRDMA_WIRE_DIRECT) != 0;
  j->links.resize(n);
  bool ok = hipEventCreate(&j->ev0) == hipSuccess && hipEventCreate(&j->ev1) == hipSuccess;
  uint64_t off = 0;
  for (uint32_t i = 0; i < n && ok; i++) {
    grdma_job_link& l = j->links[i];
    if (tx[i] && rx[i] && (tx[i]->verbs || rx[i]->verbs)) {
      // (a job's wire step is a copy kernel into the peer ring: a queue pair is posted from the host, Send by Send)
      fail(GRDMA_ERR_INVALID, "stream job link %u: a pair on the NIC wire (grdma_pair_verbs_open) cannot run a device-resident job", i);
      ok = false;
      break;
    }
    if (!tx[i] || !rx[i] || tx[i]->peer != rx[i] || !counts[i] || !rx_dsts[i] ||
        tx[i]->stream != j->stream || ((tx[i]->flags & GRDMA_WIRE_DIRECT) != 0) != j->direct) {
      fail(GRDMA_ERR_INVALID, "stream job link %u: needs two connected pairs on the shared stream", i);
      ok = false;
      break;
    }
    l.tx = tx[i];
    l.rx = rx[i];
    l.count = counts[i];
    l.dst = static_cast<uint8_t*>(rx_dsts[i]);
    l.dst_cap = rx_dst_caps[i];
    l.slices_cap = slices_caps[i];
    if (tx[i]->ring_size > j->max_ring) j->max_ring = tx[i]->ring_size;
    ok = hipMalloc((void**)&l.d_sges, sizeof(grdma_sge) * l.count) == hipSuccess &&
         hipMalloc((void**)&l.d_slices, sizeof(grdma_slice_out) * l.slices_cap) == hipSuccess &&
         hipMalloc((void**)&l.d_wireplan2, sizeof(grdma_plan)) == hipSuccess &&
         hipMalloc((void**)&l.d_rxplan2, sizeof(grdma_plan)) == hipSuccess &&
         (j->direct || hipMalloc((void**)&l.d_staging2, tx[i]->ring_size / 2 + 64) == hipSuccess) &&
         hipMalloc((void**)&l.d_encpre, sizeof(uint64_t) * (l.count + 1)) == hipSuccess &&
         hipMalloc((void**)&l.d_lenpre, sizeof(uint64_t) * (l.count + 1)) == hipSuccess &&
         hipMalloc((void**)&l.d_tilepre, sizeof(uint32_t) * (l.count + 1)) == hipSuccess;
    if (!ok) break;
    hipMemset(l.d_wireplan2, 0, sizeof(grdma_plan));
    hipMemset(l.d_rxplan2, 0, sizeof(grdma_plan));
    if (l.d_staging2) hipMemset(l.d_staging2, 0, tx[i]->ring_size / 2 + 64);
    std::vector<grdma_sge> tmp(l.count);
    for (uint64_t q = 0; q < l.count; q++) {
      tmp[q].ptr = static_cast<const uint8_t*>(slices[off + q].ptr);
      tmp[q].len = slices[off + q].len;
    }
    off += l.count;
    ok = hipMemcpy(l.d_sges, tmp.data(), sizeof(grdma_sge) * l.count, hipMemcpyHostToDevice) == hipSuccess;
  }
  // (the size tables of the rounds)
  ok = ok && hipMalloc((void**)&j->d_hints, sizeof(grdma_size_hint) * 3 * n) == hipSuccess &&
       hipMemset(j->d_hints, 0, sizeof(grdma_size_hint) * 3 * n) == hipSuccess;
  const size_t sz_tx = sizeof(grdma_tx_op) * 3 * n, sz_rx = sizeof(grdma_rx_op) * 3 * n;
  const size_t sz_txr = sizeof(grdma_tx_result) * n, sz_rxr = sizeof(grdma_rx_result) * 2 * n;
  const size_t sz_pl = sizeof(grdma_plan*) * 3 * n;
  const size_t sz_lim = sizeof(uint64_t) * 3 * n, sz_cn = sizeof(grdma_conn*) * n;
  if (ok) ok = hipMalloc((void**)&j->d_ctl, sz_tx + sz_rx + sz_txr + sz_rxr + sz_pl + sz_lim + sz_cn) == hipSuccess;
  if (!ok) {
    if (g_err.empty()) fail(GRDMA_ERR_HIP, "stream job allocation failed");
    grdma_stream_job_destroy(j);
    return nullptr;
  }
  j->d_txop = reinterpret_cast<grdma_tx_op*>(j->d_ctl);
  j->d_rxop = reinterpret_cast<grdma_rx_op*>(j->d_ctl + sz_tx);
  j->d_txres = reinterpret_cast<grdma_tx_result*>(j->d_ctl + sz_tx + sz_rx);
  j->d_rxres = reinterpret_cast<grdma_rx_result*>(j->d_ctl + sz_tx + sz_rx + sz_txr);
  j->d_plans = reinterpret_cast<const grdma_plan**>(j->d_ctl + sz_tx + sz_rx + sz_txr + sz_rxr);
  j->d_limits = reinterpret_cast<uint64_t*>(j->d_ctl + sz_tx + sz_rx + sz_txr + sz_rxr + sz_pl);
  j->d_txconns = reinterpret_cast<grdma_conn**>(j->d_ctl + sz_tx + sz_rx + sz_txr + sz_rxr + sz_pl + sz_lim);
  std::vector<uint8_t> host(sz_tx + sz_rx + sz_txr + sz_rxr + sz_pl + sz_lim + sz_cn, 0);
  auto* h_tx = reinterpret_cast<grdma_tx_op*>(host.data());
  auto* h_rx = reinterpret_cast<grdma_rx_op*>(host.data() + sz_tx);
  auto** h_pl = reinterpret_cast<const grdma_plan**>(host.data() + sz_tx + sz_rx + sz_txr + sz_rxr);
  for (int k = 0; k < 3; k++)
    for (uint32_t i = 0; i < n; i++) {
      const grdma_job_link& l = j->links[i];
      const bool odd = k == 1;
      grdma_tx_op& t = h_tx[k * n + i];
      t.conn = l.tx->d_conn;
      t.slices = l.d_sges;
      t.nslices = l.count;
      t.plan = l.tx->d_txplan;
      t.wire_plan = odd ? l.d_wireplan2 : l.tx->d_wireplan;
      t.staging_alt = odd ? l.d_staging2 : nullptr;
      t.result = &j->d_txres[i];
      t.use_cursor = k == 0 ? 2 : 1;
      t.tail_out = &j->d_limits[k * n + i];
      t.sizes_out = &j->d_hints[k * n + i];
      grdma_rx_op& r = h_rx[k * n + i];
      r.conn = l.rx->d_conn;
      r.plan = odd ? l.d_rxplan2 : l.rx->d_rxplan;
      r.result = &j->d_rxres[(odd ? n : 0) + i];
      r.slices = l.d_slices;
      r.arena = l.dst;
      r.arena_cap = l.dst_cap;
      r.max_reads = GRDMA_MAX_SLICES;
      r.raw_cap = 0;
      r.append = k == 0 ? 2 : 1;
      r.slices_cap = l.slices_cap;
      r.limit_ptr = &j->d_limits[k * n + i];
      r.sizes_in = t.sizes_out;
    }
  auto** h_cn = reinterpret_cast<grdma_conn**>(host.data() + sz_tx + sz_rx + sz_txr + sz_rxr + sz_pl + sz_lim);
  for (uint32_t i = 0; i < n; i++) h_cn[i] = j->links[i].tx->d_conn;
  for (uint32_t i = 0; i < n; i++) {
    h_pl[i] = j->links[i].tx->d_txplan;
    h_pl[n + i] = j->links[i].tx->d_wireplan;   // even rounds
    h_pl[2 * n + i] = j->links[i].d_wireplan2;  // odd rounds
  }
  // the scatter plans are addressed through the rx ops; the plan pointer array is for k_copy
  if (hipMemcpy(j->d_ctl, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
    fail(GRDMA_ERR_HIP, "job control block upload failed");
    grdma_stream_job_destroy(j);
    return nullptr;
  }
  {
    std::vector<grdma_txf_ctl> h_txf(n);
    for (uint32_t i = 0; i < n; i++) {
      const grdma_job_link& l = j->links[i];
      memset(&h_txf[i], 0, sizeof(grdma_txf_ctl));
      h_txf[i].slices = l.d_sges;
      h_txf[i].n = l.count;
      h_txf[i].enc_pre = l.d_encpre;
      h_txf[i].len_pre = l.d_lenpre;
      h_txf[i].tile_pre = l.d_tilepre;
      h_txf[i].tile_shift = GRDMA_PLAN_TILE_SHIFT(l.tx->ring_size);
    }
    if (hipMalloc((void**)&j->d_txf, sizeof(grdma_txf_ctl) * n) != hipSuccess ||
        hipMemcpy(j->d_txf, h_txf.data(), sizeof(grdma_txf_ctl) * n, hipMemcpyHostToDevice) != hipSuccess) {
      fail(GRDMA_ERR_HIP, "job index block allocation failed");
      grdma_stream_job_destroy(j);
      return nullptr;
    }
  }
  return j;
}

grdma_stream_job* grdma_stream_job_create(grdma_pair* tx, grdma_pair* rx,
                                          const grdma_slice* slices, uint64_t count,
                                          void* rx_dst, uint64_t rx_dst_cap,
                                          uint64_t slices_cap, uint64_t max_rounds) {
  return grdma_stream_job_create_multi(1, &tx, &rx, slices, &count, &rx_dst, &rx_dst_cap,
                                       &slices_cap, max_rounds);
}

void grdma_stream_job_destroy(grdma_stream_job* j) {
  if (!j) return;
  if (j->stream) hipStreamSynchronize(j->stream);
  if (j->exec) hipGraphExecDestroy(j->exec);
  for (hipStream_t st : {j->s_wire, j->s_rxplan, j->s_apply})
    if (st) {
      hipStreamSynchronize(st);
      hipStreamDestroy(st);
    }
  if (j->d_txf) hipFree(j->d_txf);
  if (j->d_hints) hipFree(j->d_hints);
  for (grdma_job_link& l : j->links) {
    if (l.d_encpre) hipFree(l.d_encpre);
    if (l.d_lenpre) hipFree(l.d_lenpre);
    if (l.d_tilepre) hipFree(l.d_tilepre);
  }
  for (hipEvent_t e : j->kev) hipEventDestroy(e);
  for (hipEvent_t e : j->pev) hipEventDestroy(e);
  if (j->ev0) hipEventDestroy(j->ev0);
  if (j->ev1) hipEventDestroy(j->ev1);
  for (auto& l : j->links) {
    hipFree(l.d_sges);
    hipFree(l.d_slices);
    hipFree(l.d_wireplan2);
    hipFree(l.d_rxplan2);
    hipFree(l.d_staging2);
    for (uint8_t* b : l.d_staging_n)
      if (b) hipFree(b);
  }
  hipFree(j->d_ctl);
  delete j;
}

int grdma_stream_job_set_rounds(grdma_stream_job* j, uint64_t rounds) {
  if (!j || rounds == 0) return fail(GRDMA_ERR_INVALID, "bad rounds");
  j->rounds = rounds;
  return 0;
}

int grdma_stream_job_set_pipeline(grdma_stream_job* j, int on) {
  if (!j) return fail(GRDMA_ERR_INVALID, "null job");
  j->pipeline = on ? 1 : 0;
  return 0;
}

// "Promised credit" for the paired schedule of a pipelined job on a staged wire (csrc/grdma_rx_plan.hip, k_plan_pair_mw): the
// Send of round t + 1 is priced with the credit the drain of round t is going to post -- it waits for that drain's plan
// inside the launch they share -- so a ring that every round fills (the reference's default: 4 MiB) carries a full round
// every round, as on the sequential schedule, in three launches instead of five.
int grdma_stream_job_set_promised_credit(grdma_stream_job* j, int on) {
  if (int rc = require_ctx()) return rc;
  if (!j) return fail(GRDMA_ERR_INVALID, "null job");
  j->promise = on != 0;
  return 0;
}

int grdma_stream_job_set_fused_wire(grdma_stream_job* j, int on) {
  if (int rc = require_ctx()) return rc;
  if (!j) return fail(GRDMA_ERR_INVALID, "null job");
  j->fuse_wire = on != 0;  // (part of job_fastkey: the graph is rebuilt)
  return 0;
}
uint32_t grdma_stream_job_wire_groups(grdma_stream_job* j) {
  if (!j || !job_is_paired(j)) return 0;
  return job_wire_groups(j);
}

int grdma_stream_job_set_rebuild_index(grdma_stream_job* j, int on) {
  if (int rc = require_ctx()) return rc;
  if (!j) return fail(GRDMA_ERR_INVALID, "null job");
  if (j->sges_exposed == (on != 0)) return 0;
  HIP_TRY(hipStreamSynchronize(j->stream));
  j->sges_exposed = on != 0;      // (job_index_needed: the graph is captured with k_tx_index in front of round 0)
  j->index_valid = false;
  if (j->exec) hipGraphExecDestroy(j->exec);
  j->exec = nullptr;
  return 0;
}

// `sends` consecutive Sends per round in ONE plan (1 = the plain schedule): what rdma_flush does while the ring has
// room -- Send, advance the cursor, Send again (rdma_bp_posix.cc:470-524) -- priced by the planners of
// csrc/grdma_tx_multi.h from the index, Send k + 1 from the state Send k leaves; the peer drains once per round.  For
// the paired schedule with the small planner workgroups (the default of a pipelined job); other schedules keep one
// Send per round.  The staging buffers of both parities then hold `sends` x ring / 2 bytes.
int grdma_stream_job_set_sends(grdma_stream_job* j, uint32_t sends) {
  if (int rc = require_ctx()) return rc;
  if (!j || sends == 0 || sends > grdma_tx_multi_max_sends()) return fail(GRDMA_ERR_INVALID, "sends must be 1..%u", grdma_tx_multi_max_sends());
  if (sends == j->sends) return 0;
  const uint32_t n = (uint32_t)j->links.size();
  HIP_TRY(hipStreamSynchronize(j->stream));
  for (uint32_t i = 0; i < n; i++) {
    grdma_job_link& l = j->links[i];
    if (!j->direct && sends > 1) {
      // (the Sends of a round are limited by the free space of the ring: a ring's worth of staging is enough)
      const size_t bytes = (size_t)l.tx->ring_size + 64;
      for (int q = 0; q < 2; q++) {
        if (l.d_staging_n[q]) continue;
        HIP_TRY(hipMalloc((void**)&l.d_staging_n[q], bytes));
        HIP_TRY(hipMemset(l.d_staging_n[q], 0, bytes));
      }
    }
    for (int k = 0; k < 3; k++) {
      uint8_t* alt = (sends > 1 && !j->direct) ? l.d_staging_n[k == 1 ? 1 : 0] : (k == 1 ? l.d_staging2 : nullptr);
      HIP_TRY(hipMemcpy(&j->d_txop[k * n + i].staging_alt, &alt, sizeof(alt), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(&j->d_txf[i].sends, &sends, sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  j->sends = sends;
  j->index_valid = false;  // (built again by the next run's first round)
  return 0;
}

namespace {
// (re)build the executable graph when the job's shape changed: rounds, schedule, which planner kernels it uses
int job_ensure_exec(grdma_stream_job* j) {
  if (!job_exec_stale(j)) return 0;
  if (j->exec) {
    HIP_TRY(hipStreamSynchronize(j->stream));
    hipGraphExecDestroy(j->exec);
  }
  j->exec = nullptr;
  hipGraph_t graph;
  if (int rc = job_build_graph(j, &graph)) return rc;
  HIP_TRY(hipGraphInstantiate(&j->exec, graph, nullptr, nullptr, 0));
  hipGraphDestroy(graph);
  j->exec_rounds = j->rounds;
  j->exec_pipeline = j->pipeline;
  j->exec_fastkey = job_fastkey(j);
  j->exec_hooks_gen = j->hooks_gen;
  return 0;
}
}  // namespace

int grdma_stream_job_run(grdma_stream_job* j, int mode, grdma_stream_result* out) {
  if (int rc = require_ctx()) return rc;
  if (!j || !out) return fail(GRDMA_ERR_INVALID, "null argument");
  hipStream_t s = j->stream;
  const size_t n = j->links.size();
  std::vector<grdma_conn> c0t(n), c0r(n), c1t(n), c1r(n);
  for (size_t i = 0; i < n; i++) {
    if (int rc = fetch_conn(j->links[i].tx, &c0t[i])) return rc;
    if (int rc = fetch_conn(j->links[i].rx, &c0r[i])) return rc;
  }
  memset(out, 0, sizeof(*out));
  if (mode == GRDMA_RUN_GRAPH) {
    if (int rc = job_ensure_exec(j)) return rc;
    HIP_TRY(hipEventRecord(j->ev0, s));
    HIP_TRY(hipGraphLaunch(j->exec, s));
    HIP_TRY(hipEventRecord(j->ev1, s));
  } else {
    HIP_TRY(hipEventRecord(j->ev0, s));
    if (mode == GRDMA_RUN_INSTRUMENTED_SCHEDULE) {
      if (!job_is_paired(j))
        return fail(GRDMA_ERR_INVALID, "GRDMA_RUN_INSTRUMENTED_SCHEDULE times the paired schedule (pipelined job, steady-state planners)");
      if (int rc = job_enqueue_chain(j, JOB_PAIRED, true, s, true)) return rc;
    } else if (j->pipeline && mode == GRDMA_RUN_EAGER && !j->promise) {
      // (a promised-credit job's eager pass runs in order instead: the stream pipeline sees its credit a round late,
      //  the graph of such a job does not)
      if (int rc = job_enqueue_streams(j, s)) return rc;
    } else {
      if (int rc = job_enqueue_chain(j, JOB_SEQUENTIAL, false, s, mode == GRDMA_RUN_INSTRUMENTED)) return rc;
    }
    HIP_TRY(hipEventRecord(j->ev1, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, j->ev0, j->ev1));
  out->ms_total = ms;
  if (mode == GRDMA_RUN_INSTRUMENTED_SCHEDULE || mode == GRDMA_RUN_INSTRUMENTED) {
    for (size_t e = 0; e < j->kev_cls.size(); e++) {  // (the timed chain: event e in front of, e + 1 behind, launch e)
      float t = 0;
      HIP_TRY(hipEventElapsedTime(&t, j->kev[e], j->kev[e + 1]));
      out->ms_class[j->kev_cls[e]] += t;
      out->launches_class[j->kev_cls[e]]++;
    }
  }
  out->done = 1;
  for (size_t i = 0; i < n; i++) {
    if (int rc = fetch_conn(j->links[i].tx, &c1t[i])) return rc;
    if (int rc = fetch_conn(j->links[i].rx, &c1r[i])) return rc;
    const uint64_t sent = c1t[i].total_written - c0t[i].total_written;
    const uint64_t deliv = c1r[i].total_read - c0r[i].total_read;
    out->bytes_sent += sent;
    out->bytes_delivered += deliv;
    out->slices_delivered += c1r[i].rx_slice_idx;
    out->tx_rounds = std::max<uint64_t>(out->tx_rounds, c1t[i].tx_rounds - c0t[i].tx_rounds);
    out->rx_rounds = std::max<uint64_t>(out->rx_rounds, c1r[i].rx_rounds - c0r[i].rx_rounds);
    out->tx_records += c1t[i].tx_records - c0t[i].tx_records;
    out->rx_records += c1r[i].rx_records - c0r[i].rx_records;
    if (!(c1t[i].tx_slice_idx >= j->links[i].count && deliv == sent)) out->done = 0;
  }
  // The job kernels try the steady-state bodies first and run the general planners (under a quarter of their
  // register budget) for what those decline.  A job whose last drains / Send keep being declined -- no period in
  // its record sizes, Sends cut by the staging budget, ... -- goes back to the plain planner kernels.
  j->runs++;
  // (round 0 of this run built the index -- only a schedule that prices its Sends from it launches k_tx_index: a run
  //  on the general send planner leaves the index as it was)
  if (j->tx_fast && j->rounds >= 1) j->index_valid = true;
  // (not with several Sends per plan: only the small planner workgroups price those, and what they decline is planned
  //  by the general planners inside the same launch, at their full register budget)
  if (j->sends == 1 && !j->promise && j->rounds >= 2 && (j->rx_fast || j->tx_fast)) {
    uint64_t cnt[3][2];  // {taken, declined with work waiting} of link 0: drains of both parities, Sends
    uint32_t c32[2][2];  // {pad1 = taken, pad0 = declined}
    static_assert(offsetof(grdma_rx_result, pad0) == offsetof(grdma_rx_result, pad1) + 4, "layout");
    HIP_TRY(hipMemcpy(c32[0], &j->d_rxres[0].pad1, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c32[1], &j->d_rxres[n].pad1, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int q = 0; q < 2; q++) { cnt[q][0] = c32[q][0]; cnt[q][1] = c32[q][1]; }
    HIP_TRY(hipMemcpy(cnt[2], &j->d_txres[0].dbg[10], 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const uint64_t rx_took = cnt[0][0] + cnt[1][0], rx_decl = cnt[0][1] + cnt[1][1];
    const uint64_t d_rx_took = rx_took - j->seen[0], d_rx_decl = rx_decl - j->seen[1];
    const uint64_t d_tx_took = cnt[2][0] - j->seen[2], d_tx_decl = cnt[2][1] - j->seen[3];
    j->seen[0] = rx_took; j->seen[1] = rx_decl; j->seen[2] = cnt[2][0]; j->seen[3] = cnt[2][1];
    // a miss: the run's drains (Sends) with work waiting went to the general planner, more than a start-up's worth
    if (d_rx_took + d_rx_decl) j->rx_miss = d_rx_decl > 2 + d_rx_took ? j->rx_miss + 1 : 0;
    if (d_tx_took + d_tx_decl) j->tx_miss = d_tx_decl > 2 + d_tx_took ? j->tx_miss + 1 : 0;
    if (j->rx_fast && j->rx_miss >= 2) j->rx_fast = 0;
    if (j->tx_fast && j->tx_miss >= 2) j->tx_fast = 0;
  }
  return 0;
}

int grdma_pair_debug_hist(grdma_pair* p, uint32_t* hist_out, uint64_t* count, uint32_t* period) {
  if (!p) return -1;
  grdma_conn c;
  if (int rc = fetch_conn(p, &c)) return rc;
  hipMemcpy(hist_out, p->d_hist, sizeof(uint32_t) * GRDMA_RX_HIST, hipMemcpyDeviceToHost);
  *count = c.rx_hist_count;
  *period = c.rx_period;
  return 0;
}

int grdma_stream_job_debug(grdma_stream_job* j, uint64_t* tx_dbg, uint64_t* rx_dbg) {
  if (!j) return -1;
  hipStreamSynchronize(j->stream);
  // result blocks alternate between even and odd rounds: GRDMA_DBG_ODD=1 shows the last odd round
  // (with 9 rounds per step the last even round is the short ninth one)
  const size_t slot = getenv("GRDMA_DBG_ODD") ? j->links.size() : 0;
  hipMemcpy(tx_dbg, j->d_txres[slot].dbg, sizeof(uint64_t) * 16, hipMemcpyDeviceToHost);
  hipMemcpy(rx_dbg, j->d_rxres[slot].dbg, sizeof(uint64_t) * 16, hipMemcpyDeviceToHost);
  return 0;
}

int grdma_stream_job_launch(grdma_stream_job* j) {
  if (int rc = require_ctx()) return rc;
  if (!j) return fail(GRDMA_ERR_INVALID, "null job");
  if (!j->exec) return fail(GRDMA_ERR_INVALID, "run the job once in GRDMA_RUN_GRAPH mode before launching it");
  if (int rc = job_ensure_exec(j)) return rc;  // (the last run may have switched the job to other planner kernels)
  HIP_TRY(hipGraphLaunch(j->exec, j->stream));
  return 0;
}

// What the HTTP/2 pipe (grdma_h2.hip) needs from a job: the device tables of one link and the
// stream the job's launches go to.
extern "C" __attribute__((visibility("hidden"))) int grdma_job_link_view(grdma_stream_job* j, uint32_t link, grdma_sge** d_sges,
                                                                         uint64_t* count, grdma_slice_out** d_slices,
                                                                         uint8_t** dst, hipStream_t* stream) {
  if (!j || link >= j->links.size()) return -1;
  grdma_job_link& l = j->links[link];
  j->sges_exposed = true;  // (the caller may rewrite the table: its index is rebuilt at every step from now on)
  *d_sges = l.d_sges;
  *count = l.count;
  *d_slices = l.d_slices;
  *dst = l.dst;
  *stream = j->stream;
  return 0;
}

// How many links the job has, and where a step leaves the number of slices it delivered on one of them: the device
// word the drain planners keep (grdma_conn::rx_slice_idx of the receiving end) and the capacity of the link's slice
// table.  Nothing of the job changes (grdma_job_link_view marks the tables as rewritable).
extern "C" __attribute__((visibility("hidden"))) uint32_t grdma_job_link_count(grdma_stream_job* j) {
  return j ? (uint32_t)j->links.size() : 0;
}
extern "C" __attribute__((visibility("hidden"))) int grdma_job_link_step_slices(grdma_stream_job* j, uint32_t link,
                                                                                const uint64_t** d_count, uint64_t* cap) {
  if (!j || link >= j->links.size()) return -1;
  const grdma_job_link& l = j->links[link];
  *d_count = reinterpret_cast<const uint64_t*>(reinterpret_cast<const uint8_t*>(l.rx->d_conn) + offsetof(grdma_conn, rx_slice_idx));
  *cap = l.slices_cap;
  return 0;
}

// Kernel nodes in front of and behind the job INSIDE its graph (one launch per step, no graph boundary -- ~15-20 us of
// idle device each -- between the stages); null / 0 removes them.  The graph is rebuilt at the next launch.
// Hooks are PER JOB and ASSIGNED, not added: a second caller replaces the first one's kernels, whichever link either
// of them works on.  A stage that serves several links of one job is one hook over a table of links (the HTTP/2 group
// pipe); who must not replace somebody else's hooks asks grdma_job_hook_counts first.
extern "C" __attribute__((visibility("hidden"))) int grdma_job_set_hooks(grdma_stream_job* j, const grdma_job_hook* pre,
                                                                         uint32_t n_pre, const grdma_job_hook* post,
                                                                         uint32_t n_post) {
  if (!j) return -1;
  j->pre_hooks.assign(pre, pre + (pre ? n_pre : 0));
  j->post_hooks.assign(post, post + (post ? n_post : 0));
  j->hooks_gen++;
  return 0;
}

// out = {pre hooks, post hooks} the job's graph carries.  Not part of include/grdma_amd.h: for the stages that hang
// hooks into a job (csrc/grdma_h2.hip) and for their tests.
int grdma_job_hook_counts(grdma_stream_job* j, uint32_t out[2]) {
  if (!j || !out) return fail(GRDMA_ERR_INVALID, "null job");
  out[0] = (uint32_t)j->pre_hooks.size();
  out[1] = (uint32_t)j->post_hooks.size();
  return 0;
}

int grdma_stream_job_launch_streams(grdma_stream_job* j) {
  if (int rc = require_ctx()) return rc;
  if (!j) return fail(GRDMA_ERR_INVALID, "null job");
  // (unlike GRDMA_RUN_EAGER this does not look at the promised credit)
  return j->pipeline ? job_enqueue_streams(j, j->stream) : job_enqueue_chain(j, JOB_SEQUENTIAL, false, j->stream, false);
}

int grdma_stream_job_sync(grdma_stream_job* j) {
  if (int rc = require_ctx()) return rc;
  if (!j) return fail(GRDMA_ERR_INVALID, "null job");
  HIP_TRY(hipStreamSynchronize(j->stream));
  return 0;
}

// Delivered slices {offset into the link's destination, length} of link `link`.
int grdma_stream_job_slices_of(grdma_stream_job* j, uint32_t link, grdma_read_slice* out, uint64_t cap) {
  if (int rc = require_ctx()) return rc;
  if (!j || !out || link >= j->links.size()) return fail(GRDMA_ERR_INVALID, "bad argument");
  grdma_conn c;
  if (int rc = fetch_conn(j->links[link].rx, &c)) return rc;
  uint64_t n = c.rx_slice_idx < cap ? c.rx_slice_idx : cap;
  static_assert(sizeof(grdma_read_slice) == sizeof(grdma_slice_out), "layout");
  if (n) HIP_TRY(hipMemcpy(out, j->links[link].d_slices, sizeof(grdma_slice_out) * n, hipMemcpyDeviceToHost));
  return (int)n;
}

int grdma_stream_job_slices(grdma_stream_job* j, grdma_read_slice* out, uint64_t cap) {
  return grdma_stream_job_slices_of(j, 0, out, cap);
}

}  // extern "C"
