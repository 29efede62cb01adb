// The bodies of the windowed reply's two stages as source text, included by the single-transport kernels (k_h2_wr_*)
// and by the many-link kernels (k_h2_links_wr_*: workgroup l is link l), csrc/grdma_h2_wr.h.  H2WR_STAGE selects the
// stage; both expect `h2wr_dev* W` in scope, as the single kernels' parameter is.
// (Source text rather than device functions, as csrc/grdma_h2_sw_stage.inc.)
#if H2WR_STAGE == 1  // k_h2_wr_queue
  __shared__ uint64_t s_wave[H2WR_THREADS / 64];
  const uint64_t tid = threadIdx.x;
  const h2r_dev* R = W->R;
  h2sw_dev* F = W->F;
  const h2a_dev* A = R->src;
  const grdma_h2_stream_dev* map = F->gp->tab;  // the map of the transport the replies go OUT on
  const uint32_t map_mask = F->gp->tab_mask;
  const uint32_t cur = W->cur & 1u;
  const grdma_h2_msg_dev* om = W->msgs[cur];
  const uint64_t* op = W->prog[cur];
  const uint64_t* ork = W->rank[cur];
  grdma_h2_msg_dev* nm = W->msgs[cur ^ 1u];
  uint64_t* np = W->prog[cur ^ 1u];
  uint64_t* nrk = W->rank[cur ^ 1u];
  const uint64_t cap = W->max_pending;
  // 1. what waited: unfinished, and the peer has neither reset nor finished its stream; compacted in the queue's order
  const uint64_t nq = W->nq < cap ? W->nq : cap;
  uint64_t kept = 0, my_closed = 0, my_status = 0, my_unrouted = 0;
  for (uint64_t q0 = 0; q0 < nq; q0 += H2WR_THREADS) {
    const uint64_t i = q0 + tid;
    uint64_t keep = 0, p = 0, rk = 0;
    grdma_h2_msg_dev m{nullptr, 0, 0, 0};
    if (i < nq) {
      m = om[i];
      p = op[i];
      rk = ork[i];
      if (p < 5 + m.len) {
        if (tab_find(map, map_mask, m.stream_id) >= 0) keep = 1;
        else my_closed++;  // (even one that is partly sent: it can never be granted)
      }
    }
    uint64_t tot;
    const uint64_t x = h2wr_block_scan(keep, s_wave, &tot);
    if (keep) {  // (kept + x < nq <= cap)
      nm[kept + x] = m;
      np[kept + x] = p;
      nrk[kept + x] = rk;
    }
    kept += tot;
  }
  // 2. what just arrived: the kept descriptors of the source's last call, by the rules of k_h2_reply_plan, progress 0
  const bool bad = W->take && (A->skip != 0 || A->ndesc > A->desc_cap || A->ndesc > R->max_messages);
  const uint64_t nd = (W->take && !bad) ? A->ndesc : 0;
  const grdma_h2_rx_msg* desc = A->desc;
  const uint64_t n_old = kept;
  for (uint64_t d0 = 0; d0 < nd; d0 += H2WR_THREADS) {
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
        } else if (tab_find(map, map_mask, to) < 0) {
          my_closed++;
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
    const uint64_t x = h2wr_block_scan(keep, s_wave, &tot);
    if (keep && kept + x < cap) {  // (beyond: the queue is full, the count below says by how much)
      nm[kept + x] = m;
      np[kept + x] = 0;
      nrk[kept + x] = A->rank_base + i;
    }
    kept += tot;
  }
  uint64_t n_status, n_unrouted, n_closed;
  h2wr_block_scan(my_status, s_wave, &n_status);
  h2wr_block_scan(my_unrouted, s_wave, &n_unrouted);
  h2wr_block_scan(my_closed, s_wave, &n_closed);
  if (tid == 0) {
    const uint64_t over = bad ? 1 : (kept > cap ? 2 : 0);
    W->n_tab = over ? 0 : kept;
    W->n_new = kept - n_old;
    W->n_status = n_status;
    W->n_unrouted = n_unrouted;
    W->n_closed = n_closed;
    W->count = kept;
    W->over = over;
    // the plan's table for this call; after an overflow it frames nothing and no window moves
    F->msgs = nm;
    F->prog_in = np;
    F->nmsgs = over ? 0 : kept;
  }
#elif H2WR_STAGE == 2  // k_h2_wr_commit
  __shared__ uint64_t s_wave[H2WR_THREADS / 64];
  __shared__ unsigned long long s_oldest;
  const uint64_t tid = threadIdx.x;
  h2sw_dev* F = W->F;
  const h2a_dev* A = W->R->src;
  const uint64_t over = W->over ? W->over : (F->fres[H2SW_F_OVERFLOW] ? 1 : 0);
  // the table that is current behind the call: the new one, or after an overflow the one that stands
  const uint32_t at = over ? (W->cur & 1u) : ((W->cur & 1u) ^ 1u);
  const uint64_t n = over ? (W->nq < W->max_pending ? W->nq : W->max_pending) : W->n_tab;
  const grdma_h2_msg_dev* msgs = W->msgs[at];
  uint64_t* prog = W->prog[at];
  const uint64_t* rank = W->rank[at];
  const uint64_t* after = F->prog_out;
  if (tid == 0) s_oldest = ~0ull;
  __syncthreads();
  uint64_t pending = 0;
  unsigned long long oldest = ~0ull;
  for (uint64_t i = tid; i < n; i += H2WR_THREADS) {
    uint64_t p;
    if (over) {
      p = prog[i];
    } else {
      p = after[i];
      prog[i] = p;  // (the queue's own words)
    }
    if (p < 5 + msgs[i].len) {
      pending++;
      const unsigned long long rk = rank[i];
      if (rk < oldest) oldest = rk;
    }
  }
  if (oldest != ~0ull) atomicMin(&s_oldest, oldest);
  uint64_t n_pending;
  h2wr_block_scan(pending, s_wave, &n_pending);  // (its barriers stand behind the atomics)
  if (tid != 0) return;
  if (W->lost_now) W->lost = 1;
  // What may be released: the reported messages in front of the oldest entry still pending -- and in front of a source
  // call that is new but was not taken (a skipped call reported nothing: rank_base is the call's before it).
  const bool stays = W->untaken || (W->take && over);
  uint64_t lim = (stays && !A->skip) ? A->rank_base : A->reported;
  if (s_oldest < lim) lim = s_oldest;
  const uint64_t releasable = lim > A->released ? lim - A->released : 0;
  if (!over) {
    W->cur = at;
    W->nq = n;
  }
  W->res[H2WR_FINISHED] = over ? 0 : n - n_pending;
  W->res[H2WR_PENDING] = over == 2 ? W->count : n_pending;
  W->res[H2WR_SLICES] = F->fres[H2SW_F_SLICES];
  W->res[H2WR_HDR] = F->fres[H2SW_F_HDR];
  W->res[H2WR_WIRE] = F->fres[H2SW_F_WIRE];
  W->res[H2WR_GRANTED] = over ? 0 : F->fres[H2SW_F_GRANTED];
  W->res[H2WR_STALL] = F->fres[H2SW_F_STALL];
  W->res[H2WR_OVERFLOW] = over;
  W->res[H2WR_TAKEN] = over ? 0 : W->n_new;
  W->res[H2WR_DROPPED_STATUS] = over ? 0 : W->n_status;
  W->res[H2WR_UNROUTED] = over ? 0 : W->n_unrouted;
  W->res[H2WR_CLOSED] = over ? 0 : W->n_closed;
  W->res[H2WR_RELEASABLE] = releasable;
  W->res[H2WR_FLAGS] = W->lost ? H2WR_FLAG_LOST : 0;
  W->res[H2WR_US] = 0;  // (the host's)
  W->res[H2WR_SPARE] = 0;
#else
#error "H2WR_STAGE: 1 queue, 2 commit"
#endif
