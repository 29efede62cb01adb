// Planner kernels of the streaming job: k_plan_pair_mw (drain plan of round t + send plan of round t + 1 as many small workgroups), k_rx_plan_mw.
// (device code, textually included by grdma_rx_plan.hip inside its unnamed namespace: the plan bodies it calls are there)
// ----------------------------------------------------------------------------
// k_plan_pair_mw: the planner pair of a streaming job's round as MANY small workgroups: the drain of round t laid out by
// G workgroups of four wavefronts (grdma_rx_multi.h: one record per thread, nothing exchanged between the workgroups
// but the arrival word), the Send of round t + 1 by H more (grdma_tx_multi.h).  gridDim.y = G + H; txops == nullptr:
// the last round, no Send (H = 0).  A 1024-thread planner is sixteen waves on one CU: four per SIMD, which issues one
// wave-instruction every four cycles -- 16 x (instructions per thread) cycles whatever the memory system does; here
// every SIMD has one wave and the probe / the plan stores of a round go through sixteen CUs' memory pipes.  The last
// workgroup to arrive commits, or -- if any of them declined -- runs the general planner right here (a 256-thread body
// with the whole register file: no spills, unlike behind the 1024-thread job kernels).
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(PLAN_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_plan_pair_mw(const grdma_rx_op* rxops, const grdma_tx_op* txops, const grdma_txf_ctl* ctls, uint32_t G_mode,
                    grdma_plan* const* wplans) {
  static_assert(RXM_THREADS == PLAN_THREADS && TXM_THREADS == PLAN_THREADS, "one workgroup shape for all planner bodies");
  // G_mode = receive workgroups per link | "promised credit" << 16 | wire workgroups per link << 20.
  // Promised credit: the Send waits for the drain plan of this launch and is priced with the credit that drain's scatter
  // will post (txm_body).  The hand-over: the thread that commits the drain moves grdma_plan::promise 0 -> "kept" with
  // the credit IN the word (one device-scope compare-and-swap, no cache operation) as soon as it knows the credit,
  // before its bookkeeping; the Send's workgroups poll it (bounded).  A wait that runs out moves the word 0 -> "given
  // up" instead and the WHOLE Send is priced without the promise (csrc/grdma_devfn.h: promise_keep / promise_wait /
  // promise_leave).
  // Wire workgroups (round 6; wplans != nullptr, a job of few links with small rings -- grdma_host_job.inc, job_wire_groups):
  // the WIRE of the round the drain walks rides in this launch instead of one of its own -- W workgroups per link move
  // the wire plan (what k_copy does) while the drain's workgroups load their state and lay the size table out; those
  // wait for the last wire workgroup before they look at the ring (csrc/grdma_rx_multi.h: wire_arrive / wire_wait).  A
  // round is two launches then, and the drain's first 4-5 us run under the wire's.
  // Dispatch order is blockIdx.y order: wire workgroups first, then the drain's, then the Send's -- who waits comes
  // after whom it waits for, and every wait is bounded (the invariant: grdma_host_job.inc, above job_promise).
  const uint32_t Wn = wplans != nullptr ? (G_mode >> 20) : 0u;
  const uint32_t G = G_mode & 0xFFFFu;
  if (blockIdx.y < Wn) {
    grdma_plan* const wp = wplans[blockIdx.x];
    run_plan<256, true>(wp, (blockIdx.y * PLAN_THREADS + threadIdx.x) >> 6, (Wn * PLAN_THREADS) >> 6, (int)(threadIdx.x & 63));
    __syncthreads();
    if (threadIdx.x == 0) wire_arrive(wp);
    return;
  }
  const uint32_t by = blockIdx.y - Wn, ny = gridDim.y - Wn;  // (this workgroup among the planners)
  const bool promise = ((G_mode >> 16) & 1u) != 0 && G != 0 && ny > G;
  if (by < G) {
    // a connection whose record sizes have a period: predicted from the pattern; none, but the round carries the sizes its
    // own Send computed: predicted from those (grdma_rx_hint.h).  Either way every record is verified in the ring.
    const grdma_rx_op& rop = rxops[blockIdx.x];
    ring_behind_wire ring_wait = {Wn ? wplans[blockIdx.x] : nullptr, Wn, G, false};
    credit_promised publish = {promise ? rop.plan : nullptr, ny - G + 1, false};
    rxh_pre pre;  // (the size table of the round, requested now: grdma_rx_hint.h)
    rxh_preload(rop, pre);
    // (<true>: every workgroup's own entries write-through -- the general planner may rewrite them below)
    int r = rxm_body<true>(rop, by, G, &ring_wait, &publish);
    if (r == 3) {  // (uniform over the whole grid: no workgroup has arrived yet)
      __syncthreads();
      r = rxh_body<true>(rop, by, G, &pre, &ring_wait, &publish);
    }
    if (r == 0) return;  // (uniform: not the committing workgroup)
    if (r == 2) {
      rx_plan_body(rxops[blockIdx.x]);
      if (threadIdx.x == 0) rxops[blockIdx.x].result->dbg[9] = 0;
    }
    if (promise) {
      // (a drain the general planner laid out: its credit words from the result block, written by this workgroup --
      //  read past the L1; a drain a steady-state body committed has published already)
      __syncthreads();
      if (threadIdx.x == 0) publish(xwg_ld64<true>(&rop.result->credit_sent), xwg_ld64<true>(&rop.result->credit_head));
    }
  } else {
    // (the wait for the drain's plan sits INSIDE the Send's first pricing, behind the loads that do not need the credit:
    //  csrc/grdma_tx_multi.h, take_promise)
    const grdma_rx_op* const rop_p = &rxops[blockIdx.x];
    const uint32_t Gc = G, Hc = ny - G;
    auto wait_promise = [promise, rop_p, Gc, Hc, by]() -> txm_promise {
      if (!promise) return txm_promise{false, 0, 0};
      // (g_promise_wait_dbg: a test makes the wait of every other Send workgroup run out at once)
      const uint32_t dbg = g_promise_wait_dbg;
      const uint32_t bound = (dbg != 0 && (((by - Gc) & 1u) || Hc == 1)) ? dbg - 1u : (1u << 18);  // (a single Send workgroup: its own)
      const uint64_t word = promise_wait(rop_p->plan, bound, Hc + 1);
      if ((word & 3u) == GRDMA_PROMISE_KEPT) return txm_promise{true, (word >> 2) & 1u, (word & ~GRDMA_PROMISE_RAN_OUT) >> 3};
      if (threadIdx.x == 0 && (word & GRDMA_PROMISE_RAN_OUT)) atomicAdd(&g_tx_promise[3], 1ull);  // (once per launch: the workgroup whose compare-and-swap gave it up)
      // (given up: EVERY workgroup of this Send prices with the credit posted so far -- the paired schedule's rule)
      return txm_promise{false, 0, 0};
    };
    // (the index window of the pricing lives in the LDS of the general receive planner: no drain runs in this workgroup)
    static_assert(sizeof(txm_win) <= sizeof(rx_lds), "the index window fits the receive planner's LDS");
    const int t = txm_body(txops[blockIdx.x], &ctls[blockIdx.x], by - G, ny - G, wait_promise,
                           reinterpret_cast<txm_win*>(rx_lds_get()));
    if (t == 0) return;  // (uniform)
    if (t != 2) return;
    tx_plan_body(txops[blockIdx.x]);
    if (threadIdx.x == 0) txops[blockIdx.x].result->dbg[9] = 0;
  }
}

// ----------------------------------------------------------------------------
// k_rx_plan_mw: the drain plan alone as many small workgroups (gridDim.y = G: grdma_rx_multi.h, the general planner in
// the committing workgroup for what that declines) -- an asynchronous endpoint's drains (grdma_endpoint_read_submit),
// which walk up to the connection's arrival report: a 1 MiB message is 130 records with a period, and the general
// planner's 30-50 us per pass was what bounded the receiving side of the endpoint vtable.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(PLAN_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_rx_plan_mw(const grdma_rx_op* rxops) {
  const grdma_rx_op& rop = rxops[blockIdx.x];
  int r = rxm_body<true>(rop, blockIdx.y, gridDim.y);
  if (r == 3) {
    __syncthreads();
    r = rxh_body<true>(rop, blockIdx.y, gridDim.y);
  }
  if (r != 2) return;  // (uniform)
  rx_plan_body(rop);
}
