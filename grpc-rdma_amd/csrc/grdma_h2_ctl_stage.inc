// The bodies of the control-reply writer's stages as source text, included by the single-transport kernels (k_h2_ctl_*:
// H2CTL_BLK = blockIdx.x, H2CTL_NBLK = H2CTL_GRID) and by the many-link kernels (k_h2_links_ctl_*: a link's share of the
// grid, H2CTL_NBLK = H2CTL_LINK_GRID; the scan one workgroup per link), csrc/grdma_h2_ctl.h.  H2CTL_STAGE selects the
// stage; every stage expects `h2ctl_dev* F` and `const h2ctl_call* call` in scope, as the single-transport kernels'
// parameters are.  (Source text rather than device functions, as csrc/grdma_h2_sw_stage.inc.)
//
// A workgroup's share of the n events is [lo, hi): contiguous, so that block order is event order.
#if H2CTL_STAGE == 1  // k_h2_ctl_last
  __shared__ uint32_t s_frame, s_done;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_frame = s_done = 0;
  __syncthreads();
  uint32_t frame = 0, done = 0;
  if (h2ctl_taken(call)) {  // (uniform)
    const uint64_t n = call->res->nevents, share = (n + H2CTL_NBLK - 1) / H2CTL_NBLK;
    const uint64_t lo = (uint64_t)H2CTL_BLK * share < n ? (uint64_t)H2CTL_BLK * share : n, hi = lo + share < n ? lo + share : n;
    for (uint64_t i = lo + tid; i < hi; i += H2CTL_THREADS) {
      const grdma_h2_event e = call->ev[i];
      if (e.kind == EV_FRAME && e.a != 0xffu) frame = (uint32_t)i + 1u;
      else if (e.kind == EV_PAYLOAD && e.c) done = (uint32_t)i + 1u;
    }
  }
  if (frame) atomicMax(&s_frame, frame);
  if (done) atomicMax(&s_done, done);
  __syncthreads();
  if (tid == 0) {
    F->blk[H2CTL_BLK].last_frame = s_frame;
    F->blk[H2CTL_BLK].last_done = s_done;
    if (H2CTL_BLK == 0) {  // (the first thread of the grid, or of the link's share)
      F->carry_out.type = 0;
      F->c_kind = H2CTL_K_NONE;
      F->c_acc = 0;
    }
  }
#elif H2CTL_STAGE == 2  // k_h2_ctl_mark
  __shared__ uint32_t s_frame, s_done, s_cnt[6], s_pa, s_ga;
  __shared__ unsigned long long s_qbytes;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    s_frame = s_done = s_pa = s_ga = 0;
    s_qbytes = 0;
  }
  if (tid < 6) s_cnt[tid] = 0;
  __syncthreads();
  if (tid < H2CTL_NBLK) {
    const uint32_t f = F->blk[tid].last_frame, d = F->blk[tid].last_done;
    if (f) atomicMax(&s_frame, f);
    if (d) atomicMax(&s_done, d);
  }
  __syncthreads();
  const uint32_t last_frame = s_frame, last_done = s_done;
  uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};  // pings, queued, rsts, SETTINGS ACKs, PING ACKs, GOAWAYs received
  uint64_t qbytes = 0, pa_acc = 0, ga_acc = 0;
  uint32_t pa_pos = 0, ga_pos = 0;
  if (h2ctl_taken(call)) {  // (uniform)
    const uint64_t n = call->res->nevents, share = (n + H2CTL_NBLK - 1) / H2CTL_NBLK;
    const uint64_t lo = (uint64_t)H2CTL_BLK * share < n ? (uint64_t)H2CTL_BLK * share : n, hi = lo + share < n ? lo + share : n;
    // the carried frame goes on over the PAYLOAD events in front of the first FRAME event: the first thread of the grid,
    // or of the link's share.  It is complete when the call holds a frame's end or a frame at all.
    if (H2CTL_BLK == 0 && tid == 0 && F->carry.type != 0 && !call->skipped) {
      h2ctl_frame f = F->carry;
      if (f.type != FT_SETTINGS) h2ctl_gather(call, f, 0, n);
      if (last_frame || last_done) {
        F->c_kind = h2ctl_kind(f);
        F->c_acc = f.acc;
      } else {
        F->carry_out = f;
      }
    }
    for (uint64_t i = lo + tid; i < hi; i += H2CTL_THREADS) {
      h2ctl_frame f;
      uint32_t stream = 0;
      const uint32_t kind = h2ctl_classify(call, i, n, last_frame, last_done, f, stream);
      if (kind == H2CTL_K_NONE) continue;
      if (kind == H2CTL_K_OPEN) {  // (at most one frame of a call)
        F->carry_out = f;
      } else if (kind == H2CTL_K_PING) {
        cnt[0]++;
      } else if (kind == H2CTL_K_SETTINGS) {
        cnt[1]++;
        qbytes += H2CTL_SETTINGS_ACK;
      } else if (kind == H2CTL_K_RST) {
        cnt[1]++;
        cnt[2]++;
        qbytes += H2CTL_RST;
      } else if (kind == H2CTL_K_GOT_SETTINGS_ACK) {
        cnt[3]++;
      } else if (kind == H2CTL_K_GOT_PING_ACK) {
        cnt[4]++;
        pa_pos = (uint32_t)i + 1u;  // (a thread's events ascend: its last one stays)
        pa_acc = f.acc;
      } else {
        cnt[5]++;
        ga_pos = (uint32_t)i + 1u;
        ga_acc = f.acc;
      }
    }
  }
  for (int k = 0; k < 6; k++)
    if (cnt[k]) atomicAdd(&s_cnt[k], cnt[k]);
  if (qbytes) atomicAdd(&s_qbytes, (unsigned long long)qbytes);
  if (pa_pos) atomicMax(&s_pa, pa_pos);
  if (ga_pos) atomicMax(&s_ga, ga_pos);
  __syncthreads();
  h2ctl_blk* B = &F->blk[H2CTL_BLK];
  if (pa_pos && pa_pos == s_pa) B->pa_acc = pa_acc;
  if (ga_pos && ga_pos == s_ga) B->ga_acc = ga_acc;
  if (tid == 0) {
    B->pings = s_cnt[0];
    B->queued = s_cnt[1];
    B->rsts = s_cnt[2];
    B->got_settings_acks = s_cnt[3];
    B->got_ping_acks = s_cnt[4];
    B->got_goaways = s_cnt[5];
    B->qbytes = s_qbytes;
    B->pa_pos = s_pa;
    B->ga_pos = s_ga;
  }
#elif H2CTL_STAGE == 3  // k_h2_ctl_scan
  __shared__ uint64_t s_wave[H2CTL_THREADS / 64];
  __shared__ uint32_t s_frame, s_done, s_pa, s_ga;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_frame = s_done = s_pa = s_ga = 0;
  __syncthreads();
  uint64_t pq = 0, rs = 0, pg = 0, qb = 0;  // (two counts a word: a call has fewer than 2^32 events)
  if (tid < H2CTL_NBLK) {
    const h2ctl_blk* B = &F->blk[tid];
    pq = (uint64_t)B->pings | ((uint64_t)B->queued << 32);
    rs = (uint64_t)B->rsts | ((uint64_t)B->got_settings_acks << 32);
    pg = (uint64_t)B->got_ping_acks | ((uint64_t)B->got_goaways << 32);
    qb = B->qbytes;
    if (B->last_frame) atomicMax(&s_frame, B->last_frame);
    if (B->last_done) atomicMax(&s_done, B->last_done);
    if (B->pa_pos) atomicMax(&s_pa, tid + 1u);
    if (B->ga_pos) atomicMax(&s_ga, tid + 1u);
  }
  uint64_t t_pq, t_rs, t_pg, t_qb;
  const uint64_t x_pq = block_excl_scan(pq, s_wave, &t_pq);
  const uint64_t x_qb = block_excl_scan(qb, s_wave, &t_qb);
  block_excl_scan(rs, s_wave, &t_rs);
  block_excl_scan(pg, s_wave, &t_pg);  // (its barriers also order the LDS maxima in front of their reads)
  if (tid < H2CTL_NBLK) {
    F->blk[tid].pre_pings = x_pq & 0xffffffffull;
    F->blk[tid].pre_qbytes = x_qb;
  }
  if (tid != 0) return;
  const bool lost = h2ctl_lost(call), failed = !lost && call->res->error != 0;
  const uint32_t ck = F->c_kind;
  const uint64_t pings = (t_pq & 0xffffffffull) + (ck == H2CTL_K_PING ? 1 : 0);
  const uint64_t queued = (t_pq >> 32) + (ck == H2CTL_K_SETTINGS ? 1 : 0);
  const uint64_t rsts = t_rs & 0xffffffffull;
  const uint64_t got_sa = (t_rs >> 32) + (ck == H2CTL_K_GOT_SETTINGS_ACK ? 1 : 0);
  const uint64_t got_pa = (t_pg & 0xffffffffull) + (ck == H2CTL_K_GOT_PING_ACK ? 1 : 0);
  const uint64_t got_ga = (t_pg >> 32) + (ck == H2CTL_K_GOT_GOAWAY ? 1 : 0);
  const uint64_t frames = pings + queued;
  const uint64_t wire = H2CTL_PING * pings + t_qb + (ck == H2CTL_K_SETTINGS ? H2CTL_SETTINGS_ACK : 0);
  const uint64_t slices = (wire + H2_INLINED - 1) / H2_INLINED;
  const bool over = !lost && !failed && (frames > F->max_replies || slices > F->cap || slices * 32 > F->hdr_cap);
  F->last_frame = s_frame;
  F->last_done = s_done;
  for (int k = 0; k < 8; k++) F->res[k] = 0;
  if (over) {  // the totals; nothing is written and nothing is committed
    F->res[H2CTL_FRAMES] = frames;
    F->res[H2CTL_SLICES] = slices;
    F->res[H2CTL_WIRE] = wire;
    F->res[H2CTL_N_SETTINGS] = queued - rsts;
    F->res[H2CTL_N_PING] = pings;
    F->res[H2CTL_N_RST] = rsts;
    F->res[H2CTL_FLAGS] = ((F->lost || call->skipped) ? H2CTL_F_LOST : 0) | (got_ga ? H2CTL_F_GOAWAY : 0);
    F->res[H2CTL_OVERFLOW] = 1;
    return;
  }
  if (lost || call->skipped) F->lost = 1;
  F->st_calls++;
  if (lost || failed) {  // nothing is written, nothing recorded; the carry goes (its frame's end was not seen)
    F->carry.type = 0;
    F->res[H2CTL_FLAGS] = F->lost ? H2CTL_F_LOST : 0;
    F->res[H2CTL_OVERFLOW] = lost ? 2 : 0;
    return;
  }
  F->carry = F->carry_out;
  F->peer[0] += got_sa;
  F->peer[1] += got_pa;
  if (got_pa) F->peer[2] = h2ctl_bswap(s_pa ? F->blk[s_pa - 1].pa_acc : F->c_acc);  // (the wire bytes as a little-endian word)
  F->peer[3] += got_ga;
  if (got_ga) {
    const uint64_t acc = s_ga ? F->blk[s_ga - 1].ga_acc : F->c_acc;
    F->peer[4] = (acc >> 32) & 0x7fffffffull;
    F->peer[5] = acc & 0xffffffffull;
    F->peer[6] = F->st_calls;
  }
  F->st_settings_acks += queued - rsts;
  F->st_ping_acks += pings;
  F->st_rsts += rsts;
  F->st_wire += wire;
  F->res[H2CTL_FRAMES] = frames;
  F->res[H2CTL_SLICES] = slices;
  F->res[H2CTL_WIRE] = wire;
  F->res[H2CTL_N_SETTINGS] = queued - rsts;
  F->res[H2CTL_N_PING] = pings;
  F->res[H2CTL_N_RST] = rsts;
  F->res[H2CTL_FLAGS] = (F->lost ? H2CTL_F_LOST : 0) | (got_ga ? H2CTL_F_GOAWAY : 0);
#elif H2CTL_STAGE == 4  // k_h2_ctl_emit
  __shared__ uint64_t s_wave[H2CTL_THREADS / 64];
  const uint64_t slices = F->res[H2CTL_SLICES], wire = F->res[H2CTL_WIRE];
  if (F->res[H2CTL_OVERFLOW] || slices == 0) return;  // (uniform) nothing half-written; a lost call has no slices
  const uint32_t tid = threadIdx.x;
  const uint64_t n = call->res->nevents, share = (n + H2CTL_NBLK - 1) / H2CTL_NBLK;
  const uint64_t lo = (uint64_t)H2CTL_BLK * share < n ? (uint64_t)H2CTL_BLK * share : n, hi = lo + share < n ? lo + share : n;
  const uint32_t last_frame = F->last_frame, last_done = F->last_done;
  const uint32_t ck = F->c_kind;
  uint8_t* hdr = F->hdr;
  const uint64_t q0 = H2CTL_PING * F->res[H2CTL_N_PING];  // the queued replies stand behind the PING ACKs
  // the replies of the workgroups in front, the carried frame's in front of all
  uint64_t base_p = F->blk[H2CTL_BLK].pre_pings + (ck == H2CTL_K_PING ? 1 : 0);
  uint64_t base_q = q0 + F->blk[H2CTL_BLK].pre_qbytes + (ck == H2CTL_K_SETTINGS ? H2CTL_SETTINGS_ACK : 0);
  if (H2CTL_BLK == 0 && tid == 0) {
    if (ck == H2CTL_K_PING && H2CTL_PING <= wire) h2ctl_write_reply(hdr, 0, ck, F->c_acc, 0);
    if (ck == H2CTL_K_SETTINGS && q0 + H2CTL_SETTINGS_ACK <= wire) h2ctl_write_reply(hdr, q0, ck, 0, 0);
  }
  for (uint64_t c0 = lo; c0 < hi; c0 += H2CTL_THREADS) {  // (uniform: the scan's barriers)
    const uint64_t i = c0 + tid;
    h2ctl_frame f;
    f.acc = 0;
    uint32_t stream = 0, kind = H2CTL_K_NONE;
    if (i < hi) kind = h2ctl_classify(call, i, n, last_frame, last_done, f, stream);
    const uint32_t len = kind == H2CTL_K_PING ? H2CTL_PING : kind == H2CTL_K_SETTINGS ? H2CTL_SETTINGS_ACK : kind == H2CTL_K_RST ? H2CTL_RST : 0;
    // (one scan for both ranks: fewer than 2^24 PING ACKs in 256 events)
    const uint64_t mine = kind == H2CTL_K_PING ? 1ull : ((uint64_t)len << 24);
    uint64_t tot;
    const uint64_t x = block_excl_scan(mine, s_wave, &tot);
    if (len) {
      const uint64_t o = kind == H2CTL_K_PING ? H2CTL_PING * (base_p + (x & 0xffffffull)) : base_q + (x >> 24);
      if (o + len <= wire) h2ctl_write_reply(hdr, o, kind, f.acc, stream);  // (cannot fail: the scan counted the same replies)
    }
    base_p += tot & 0xffffffull;
    base_q += tot >> 24;
  }
  // the slice descriptors of the 23-byte cuts
  for (uint64_t k = (uint64_t)H2CTL_BLK * H2CTL_THREADS + tid; k < slices; k += (uint64_t)H2CTL_NBLK * H2CTL_THREADS) {
    const uint64_t w0 = k * H2_INLINED;
    F->out[k] = grdma_sge{hdr + 32 * k, wire - w0 < H2_INLINED ? wire - w0 : H2_INLINED};
  }
#else
#error "H2CTL_STAGE: 1 last, 2 mark, 3 scan, 4 emit"
#endif
