// The bodies of the window ledger's stages as source text, included by the single-transport kernels (k_h2_fc_*: the grid
// is the call's, H2FC_BLK = blockIdx.x, H2FC_NBLK = gridDim.x) and by the many-link kernels (k_h2_links_fc_*: a link's
// share of the grid, or one workgroup per link), csrc/grdma_h2_fc.h.  H2FC_STAGE selects the stage; every stage expects
// `h2fc_dev* F` (the emit: `const h2fc_dev* F`) and, but for the emit, `const h2fc_call* call` in scope, as the
// single-transport kernels' parameters are.
// (Source text rather than device functions, as csrc/grdma_h2_asm_stage.inc: with included text tools/h2_isa_compare.py
// reports the five single-transport kernels `same`.)
#if H2FC_STAGE == 1  // k_h2_fc_clear
  const uint64_t t0 = (uint64_t)H2FC_BLK * H2FC_THREADS + threadIdx.x, step = (uint64_t)H2FC_NBLK * H2FC_THREADS;
  const h2fc_slot empty = {0, H2FC_NONE, H2FC_NONE, H2FC_NONE, 0, 0, 0};
  for (uint64_t s = t0; s <= F->tab_mask; s += step) F->tab[s] = empty;
  uint64_t n = call->res->overflow ? 0 : call->res->nevents;
  if (n > F->scratch_ev) n = 0;
  const uint64_t words = (n + 31) / 32;
  for (uint64_t w = t0; w < words; w += step) F->mark[w] = 0;
  if (t0 == 0) {  // (the first thread of the grid, or of the link's share)
    F->c_conn = 0;
    F->c_full = 0;
  }
#elif H2FC_STAGE == 2  // k_h2_fc_keys
  const uint64_t n = h2fc_events(F, call);
  const int lane = threadIdx.x & 63;
  uint64_t mine = 0;
  for (uint64_t i = (uint64_t)H2FC_BLK * H2FC_THREADS + threadIdx.x; i < n; i += (uint64_t)H2FC_NBLK * H2FC_THREADS) {
    const grdma_h2_event e = call->ev[i];
    if (h2fc_is_data(e)) {
      mine += e.d;  // (whatever its stream: skipped frames travelled too)
      // a slot only for a stream the map knows behind the call: one that left the map during the call has a
      // STREAM_CLOSED event and is claimed there, and DATA on ids the transport never knew must not fill the table
      if ((e.b >> 8) == 0 && e.c != 0 && tab_find(F->gp->tab, F->gp->tab_mask, e.c) >= 0) h2fc_claim(F, e.c);
    } else if ((e.kind == EV_STREAM_CLOSED || e.kind == EV_STREAM_OPEN) && e.c != 0) {
      const uint32_t s = h2fc_claim(F, e.c);
      if (s != H2FC_NONE) atomicMin(e.kind == EV_STREAM_CLOSED ? &F->tab[s].closed : &F->tab[s].opened, (uint32_t)i);
    }
  }
  const uint64_t sum = wave_incl_scan(mine, lane);
  if (lane == 63 && sum) atomicAdd(&F->c_conn, (unsigned long long)sum);
#elif H2FC_STAGE == 3  // k_h2_fc_sums
  if (h2fc_lost(F, call)) return;
  const uint64_t n = h2fc_events(F, call);
  for (uint64_t i = (uint64_t)H2FC_BLK * H2FC_THREADS + threadIdx.x; i < n; i += (uint64_t)H2FC_NBLK * H2FC_THREADS) {
    const grdma_h2_event e = call->ev[i];
    if (!h2fc_is_data(e) || (e.b >> 8) != 0 || e.c == 0) continue;
    const uint32_t s = h2fc_find(F, e.c);
    if (s == H2FC_NONE) continue;
    const uint32_t closed = F->tab[s].closed, opened = F->tab[s].opened;
    if ((uint32_t)i > closed || (opened != H2FC_NONE && (uint32_t)i < opened)) continue;
    atomicAdd(&F->tab[s].sum, (unsigned long long)e.d);
    atomicMin(&F->tab[s].first, (uint32_t)i);
  }
#elif H2FC_STAGE == 4  // k_h2_fc_finish
  __shared__ uint64_t s_ws[H2FC_ONE_THREADS / 64];
  __shared__ unsigned long long s_credit, s_first_viol;
  __shared__ uint32_t s_viol;
  __shared__ uint64_t s_conn, s_conn_inc, s_over;
  const uint32_t tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  if (h2fc_lost(F, call)) {  // (uniform) the call cannot be accounted: the flag, the report, nothing else
    if (tid == 0) {
      F->lost = 1;
      for (int k = 0; k < 8; k++) F->res[k] = 0;
      F->res[H2FC_VIOLATIONS] = H2FC_V_LOST;
      F->res[H2FC_OVERFLOW] = 2;  // (1 = a cap, 2 = the call was not accounted)
    }
    return;
  }
  const uint64_t n = h2fc_events(F, call);
  const bool dead = call->res->error != 0;
  const uint64_t stream_window = F->stream_window;
  if (tid == 0) {
    s_credit = 0;
    s_first_viol = ~0ull;
    s_viol = 0;
  }
  __syncthreads();
  // ---- per stream: delivered or not, violations, who gets a frame
  for (uint32_t t = tid; t <= F->tab_mask; t += H2FC_ONE_THREADS) {
    h2fc_slot sl = F->tab[t];
    if (sl.key == 0 || sl.first == H2FC_NONE) continue;
    if (sl.opened == H2FC_NONE && sl.closed == H2FC_NONE) {
      // nothing in the call says what the stream was: the parser's map does (unchanged by the call for this stream)
      const int idx = tab_find(F->gp->tab, F->gp->tab_mask, sl.key);
      if (idx < 0 || F->gp->tab[idx].read_closed) sl.sum = 0;
    }
    if (sl.sum > stream_window) {
      atomicAdd(&s_viol, 1u);
      atomicMin(&s_first_viol, ((unsigned long long)sl.first << 32) | sl.key);
    }
    sl.emit = sl.sum > 0 && sl.closed == H2FC_NONE && !dead;
    if (sl.sum > H2FC_MAX_INC) sl.sum = H2FC_MAX_INC;
    if (sl.emit) {
      atomicAdd(&F->mark[sl.first >> 5], 1u << (sl.first & 31));  // (one stream per event: the add sets the bit)
      atomicAdd(&s_credit, sl.sum);
    }
    F->tab[t] = sl;
  }
  // ---- the connection
  if (tid == 0) {
    const uint64_t D = F->c_conn;
    int64_t ann = F->announced;
    uint64_t viol = 0;
    if (D > 0 && (ann < 0 || D > (uint64_t)ann)) viol |= H2FC_V_CONN;
    ann -= (int64_t)D;
    const int64_t pending = (int64_t)F->conn_window - ann;
    uint64_t inc = 0;
    if (!dead && pending > 0 && (uint64_t)pending >= F->conn_threshold)
      inc = (uint64_t)pending > H2FC_MAX_INC ? H2FC_MAX_INC : (uint64_t)pending;
    F->announced = ann + (int64_t)inc;
    s_conn = inc ? 1 : 0;
    s_conn_inc = inc;
    s_over = viol;
  }
  __syncthreads();
  // ---- positions: the marks in front of every word
  const uint64_t words = (n + 31) / 32;
  uint64_t carry = 0;
  for (uint64_t w0 = 0; w0 < words; w0 += H2FC_ONE_THREADS) {
    const uint64_t w = w0 + tid;
    const uint64_t v = w < words ? (uint64_t)__builtin_popcount(F->mark[w]) : 0;
    const uint64_t incl = wave_incl_scan(v, lane);
    if (lane == 63) s_ws[wave] = incl;
    __syncthreads();
    uint64_t base = 0, tot = 0;
    for (int k = 0; k < H2FC_ONE_THREADS / 64; k++) {
      const uint64_t s = s_ws[k];
      if (k < wave) base += s;
      tot += s;
    }
    __syncthreads();
    if (w < words) F->mark_pre[w] = (uint32_t)(carry + base + incl - v);
    carry += tot;
  }
  __syncthreads();  // (mark_pre is read by other threads below)
  const uint64_t frames = s_conn + carry;
  const uint64_t wire = frames * H2FC_FRAME;
  const uint64_t slices = (wire + H2_INLINED - 1) / H2_INLINED;
  const bool over = frames > F->max_updates || slices > F->cap || slices * 32 > F->hdr_cap;
  if (!over) {
    for (uint32_t t = tid; t <= F->tab_mask; t += H2FC_ONE_THREADS) {
      const h2fc_slot sl = F->tab[t];
      if (sl.key == 0 || !sl.emit) continue;
      const uint32_t w = sl.first >> 5;
      const uint64_t pos = s_conn + F->mark_pre[w] + (uint64_t)__builtin_popcount(F->mark[w] & ((1u << (sl.first & 31)) - 1u));
      F->upd[pos] = h2fc_upd{sl.key, (uint32_t)sl.sum};
    }
    if (tid == 0 && s_conn) F->upd[0] = h2fc_upd{0, (uint32_t)s_conn_inc};
  }
  if (tid == 0) {
    const uint64_t viol = s_over | (s_viol ? H2FC_V_STREAM : 0) | (F->lost ? H2FC_V_LOST : 0);
    F->res[H2FC_FRAMES] = frames;
    F->res[H2FC_SLICES] = slices;
    F->res[H2FC_WIRE] = wire;
    F->res[H2FC_CONN_BYTES] = F->c_conn;
    F->res[H2FC_STREAM_BYTES] = s_credit;
    F->res[H2FC_VIOLATIONS] = viol;
    F->res[H2FC_FIRST_VIOLATOR] = s_viol ? (uint32_t)s_first_viol : 0;
    F->res[H2FC_OVERFLOW] = over ? 1 : 0;
    F->st_calls++;
    F->st_conn_bytes += F->c_conn;
    F->st_conn_over += (s_over & H2FC_V_CONN) ? 1 : 0;
    F->st_stream_over += s_viol;
    if (!over) {
      F->st_stream_bytes += s_credit;
      F->st_frames += frames;
    }
  }
#elif H2FC_STAGE == 5  // k_h2_fc_emit
  if (F->res[H2FC_OVERFLOW]) return;  // (nothing half-written; a lost call has no slices)
  const uint64_t frames = F->res[H2FC_FRAMES], slices = F->res[H2FC_SLICES], wire = F->res[H2FC_WIRE];
  for (uint64_t k = (uint64_t)H2FC_BLK * H2FC_THREADS + threadIdx.x; k < slices; k += (uint64_t)H2FC_NBLK * H2FC_THREADS) {
    const uint64_t w0 = k * H2_INLINED;
    const uint32_t len = (uint32_t)(wire - w0 < H2_INLINED ? wire - w0 : H2_INLINED);
    const uint64_t f0 = w0 / H2FC_FRAME;
    const uint32_t r0 = (uint32_t)(w0 - f0 * H2FC_FRAME);
    // a slice touches at most three frames
    const h2fc_upd u0 = F->upd[f0];
    uint32_t s1 = 0, i1 = 0, s2 = 0, i2 = 0;
    if (f0 + 1 < frames) {
      const h2fc_upd u = F->upd[f0 + 1];
      s1 = u.stream;
      i1 = u.inc;
    }
    if (f0 + 2 < frames) {
      const h2fc_upd u = F->upd[f0 + 2];
      s2 = u.stream;
      i2 = u.inc;
    }
    uint8_t* dst = F->hdr + 32 * k;
    uint64_t* d64 = reinterpret_cast<uint64_t*>(dst);
    d64[0] = h2fc_word(r0, 0, len, u0.stream, u0.inc, s1, i1, s2, i2);
    d64[1] = h2fc_word(r0, 8, len, u0.stream, u0.inc, s1, i1, s2, i2);
    d64[2] = h2fc_word(r0, 16, len, u0.stream, u0.inc, s1, i1, s2, i2);
    d64[3] = 0;
    F->out[k] = grdma_sge{dst, len};
  }
#endif
