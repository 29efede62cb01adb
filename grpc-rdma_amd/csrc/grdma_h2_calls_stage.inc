// The bodies of the call table's eight stages as source text, included by the single-call kernels (k_h2_calls_*: H2C_BLK =
// blockIdx.x, H2C_NBLK = H2C_GRID) and by the kernels over a table of links (k_h2_links_calls_*: a link's share of the
// grid, H2C_NBLK = H2C_LINK_GRID), csrc/grdma_h2_calls.h.  H2C_STAGE selects the stage.  A stage expects in scope, as the
// including kernel names them:
//   h2c_dev* F           the table: its entry tables, count rows, state and counters
//   const h2c_call* C    the step's words (&F->c in the single kernels, the item's words of the batch block over links)
//   uint64_t* R          the eight result words the host reads (stage 7)
// H2C_BLK is the workgroup's index within its table's grid of H2C_NBLK workgroups: every run, every stride and every row
// goes through the two.  All threads of a workgroup belong to one table, so every barrier below is uniform.
// (Source text rather than device functions, as csrc/grdma_h2_meta_stage.inc.)
#if H2C_STAGE == 1  // k_h2_calls_clear
  const uint64_t tid = (uint64_t)(H2C_BLK) * H2C_THREADS + threadIdx.x, nth = (uint64_t)(H2C_NBLK) * H2C_THREADS;
  h2c_entry* const neu = F->tab[1u - F->cur];
  const uint32_t slots = F->slots;
  const h2c_entry e0 = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const h2c_aux a0 = {H2C_NONE, H2C_NONE, 0, 0, 0, 0, 0, 0};
  for (uint64_t s = tid; s < slots; s += nth) neu[s] = e0, F->aux[s] = a0;
  for (uint64_t s = tid; s <= C->dd_mask; s += nth) C->dd[s] = h2c_dd{0, H2C_NONE};
  for (uint64_t s = tid; s < (uint64_t)(H2C_NBLK) * slots; s += nth) F->row_s[s] = 0;
  const uint32_t nk = F->nmethods + 1u;
  for (uint64_t s = tid; s < (uint64_t)(H2C_NBLK) * H2C_KEYS_MAX; s += nth)
    if (s % H2C_KEYS_MAX < nk) F->row_k[s] = 0;
  if (tid < (H2C_NBLK)) F->wins[tid] = 0, F->closes[tid] = 0, F->wg_bytes[tid] = 0;
  if (tid == 0) F->bad = ~0ull, F->nexp = 0, F->nleft = 0, F->go = 0;
#elif H2C_STAGE == 2  // k_h2_calls_claim
  const uint64_t tid = (uint64_t)(H2C_BLK) * H2C_THREADS + threadIdx.x, nth = (uint64_t)(H2C_NBLK) * H2C_THREADS;
  const h2c_entry* const old = F->tab[F->cur];
  const uint32_t mask = F->slots - 1u, nm = F->nmethods;
  for (uint64_t k = tid; k < C->nblocks; k += nth) {
    const uint32_t stream = C->meta[k].stream, word = C->meta[k].word, method = C->meta[k].method;
    uint32_t cls = H2C_CLS_NO;
    if (h2c_would_open(word, C->blocks[k].flags)) {
      const uint32_t code = (stream == 0 || (stream >> 31)) ? H2C_E_STREAM : method >= nm ? H2C_E_METHOD : 0u;
      if (code) {
        atomicMin(&F->bad, (unsigned long long)k << 8 | code);
      } else {
        const uint32_t s = h2c_find(old, mask, stream);
        if (s == H2C_NONE || (old[s].fin & H2C_EF_DEAD)) {  // (else a duplicate)
          const uint32_t d = h2c_claim(&C->dd[0].key, sizeof(h2c_dd) / 4u, (uint32_t)C->dd_mask, stream);
          if (d != H2C_NONE) {
            atomicMin(&C->dd[d].rec, (uint32_t)k);
            cls = H2C_CLS_CAND;
          }
        }
      }
    }
    C->cls[k] = cls;
  }
#elif H2C_STAGE == 3  // k_h2_calls_wins
  const uint32_t tid = threadIdx.x;
  __shared__ uint32_t s_n[H2C_THREADS / 64];
  uint64_t b0, b1;
  h2c_run(C->nblocks, H2C_BLK, H2C_NBLK, &b0, &b1);
  uint32_t n = 0;
  for (uint64_t k0 = b0; k0 < b1; k0 += H2C_THREADS) {  // (uniform)
    const uint64_t k = k0 + tid;
    bool win = false;
    if (k < b1 && C->cls[k] == H2C_CLS_CAND) {
      const uint32_t stream = C->meta[k].stream;
      uint32_t d = (stream >> 1) & (uint32_t)C->dd_mask;
      while (C->dd[d].key != stream) d = (d + 1u) & (uint32_t)C->dd_mask;  // (claimed in the stage before: it is there)
      win = C->dd[d].rec == (uint32_t)k;
      if (win) C->cls[k] = H2C_CLS_WIN;
    }
    n += (uint32_t)__builtin_popcountll(__ballot(win));
  }
  if ((tid & 63u) == 0) s_n[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
    for (uint32_t k = 0; k < H2C_THREADS / 64; k++) t += s_n[k];
    F->wins[H2C_BLK] = t;
  }
#elif H2C_STAGE == 4  // k_h2_calls_insert
  const uint32_t tid = threadIdx.x;
  __shared__ uint64_t s_wave[H2C_THREADS / 64];
  static_assert(H2C_THREADS == PLAN_THREADS, "block_excl_scan is for this workgroup size");
  const h2c_entry* const old = F->tab[F->cur];
  h2c_entry* const neu = F->tab[1u - F->cur];
  const uint64_t now = C->now;
  // the live entries of the table behind the last step
  for (uint64_t s = (uint64_t)(H2C_BLK) * H2C_THREADS + tid; s < F->slots; s += (uint64_t)(H2C_NBLK) * H2C_THREADS) {
    h2c_entry e = old[s];
    e.word |= e.fin;
    if (e.stream != 0 && !(e.fin & H2C_EF_DEAD)) h2c_put(F, neu, e, now);
  }
  // the winners of this run, in record order
  uint64_t run = 0;
  for (uint32_t w = 0; w < (H2C_BLK); w++) run += F->wins[w];
  const uint64_t room = F->slots / 2u - F->live;  // (live <= slots / 2)
  uint64_t b0, b1;
  h2c_run(C->nblocks, H2C_BLK, H2C_NBLK, &b0, &b1);
  for (uint64_t k0 = b0; k0 < b1; k0 += H2C_THREADS) {  // (uniform: the scan's barriers)
    const uint64_t k = k0 + tid;
    const bool win = k < b1 && C->cls[k] == H2C_CLS_WIN;
    uint64_t tot;
    const uint64_t rank = run + block_excl_scan(win ? 1ull : 0ull, s_wave, &tot);
    if (win && rank < room) {
      const h2m_meta_out r = C->meta[k];
      const uint64_t timeout = (uint64_t)r.timeout_lo | (uint64_t)r.timeout_hi << 32;
      uint64_t deadline = ~0ull;
      if ((r.word >> 24) & H2M_HAS_TIMEOUT) deadline = now + timeout < now ? ~0ull : now + timeout;
      const h2c_entry e = {F->serial + rank, deadline, 0, r.stream, r.method, 0, (r.word >> 16) & 0xffu, 0, 0};
      h2c_put(F, neu, e, now);
    }
    run += tot;
  }
#elif H2C_STAGE == 5  // k_h2_calls_msgs
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  h2c_entry* const neu = F->tab[1u - F->cur];
  const uint32_t mask = F->slots - 1u, nm = F->nmethods;
  uint32_t* const row_s = F->row_s + (size_t)(H2C_BLK) * F->slots;
  uint32_t* const row_k = F->row_k + (size_t)(H2C_BLK) * H2C_KEYS_MAX;
  // the closing events: the lowest LEFT and the lowest reads-closed event of an entry
  for (uint64_t j = (uint64_t)(H2C_BLK) * H2C_THREADS + tid; j < C->nev; j += (uint64_t)(H2C_NBLK) * H2C_THREADS) {
    const grdma_h2_event e = C->ev[j];
    if (e.kind != EV_STREAM_CLOSED || e.a > 1u || e.c == 0) continue;
    const uint32_t s = h2c_find(neu, mask, e.c);
    if (s != H2C_NONE) atomicMin(e.a ? &F->aux[s].left_at : &F->aux[s].rc_at, (uint32_t)j);
  }
  // the descriptors of this run, in order
  uint64_t b0, b1, bytes = 0;
  h2c_run(C->nmsgs, H2C_BLK, H2C_NBLK, &b0, &b1);
  for (uint64_t i0 = b0; i0 < b1; i0 += H2C_THREADS) {  // (uniform)
    const uint64_t i = i0 + tid;
    const bool valid = i < b1;
    uint32_t slot = H2C_NONE, key = nm, reason = 0;
    uint64_t len = 0;
    if (valid) {
      const h2c_msg m = C->msgs[i];
      len = m.length;
      if (m.status != 0) {
        reason = H2C_BAD_STATUS;
      } else {
        const uint32_t s = m.stream ? h2c_find(neu, mask, m.stream) : H2C_NONE;
        if (s == H2C_NONE) {
          reason = H2C_NO_CALL;
        } else {
          const uint32_t word = neu[s].word;
          slot = s;
          if (word & H2C_EF_EXPIRED) reason = H2C_EXPIRED_MSG;
          else if ((m.flags & 1u) && (word & 0xffu) == 0) reason = H2C_COMPRESSED_IDENTITY;
          else key = neu[s].method;
        }
      }
    }
    const bool disp = valid && reason == 0;
    uint32_t rank_s, tot_s, rank_k, tot_k;
    bool last_s, last_k;
    h2c_keyed(slot, disp, lane, &rank_s, &tot_s, &last_s);
    h2c_keyed(key, valid, lane, &rank_k, &tot_k, &last_k);
    // the waves take turns at the run's rows: what the waves in front of this one added is in the row
    for (uint32_t v = 0; v < H2C_THREADS / 64; v++) {  // (uniform)
      if (wave == v) {
        if (disp) {
          const uint32_t base = row_s[slot];
          rank_s += base;
          if (last_s) row_s[slot] = base + tot_s;
        }
        if (valid) {
          const uint32_t base = row_k[key];
          rank_k += base;
          if (last_k) row_k[key] = base + tot_k;
        }
      }
      __syncthreads();
    }
    if (disp) {
      atomicAdd((unsigned long long*)&neu[slot].bytes, (unsigned long long)len);
      atomicAdd(&F->aux[slot].nstep, 1u);
      atomicMax(&F->aux[slot].last, (uint32_t)i + 1u);
      bytes += len;
    }
    if (valid) C->mrec[i] = h2c_mrec{slot, key, disp ? rank_s : reason, rank_k};
  }
  // the run's dispatched bytes (a sum: its order is free)
  for (int d = 32; d >= 1; d >>= 1) bytes += __shfl_xor(bytes, d, 64);
  if (lane == 0 && bytes) atomicAdd((unsigned long long*)&F->wg_bytes[H2C_BLK], (unsigned long long)bytes);
#elif H2C_STAGE == 6  // k_h2_calls_cols
  const uint32_t tid = threadIdx.x;
  const uint64_t gid = (uint64_t)(H2C_BLK) * H2C_THREADS + tid, nth = (uint64_t)(H2C_NBLK) * H2C_THREADS;
  const h2c_entry* const neu = F->tab[1u - F->cur];
  const uint32_t slots = F->slots, nk = F->nmethods + 1u;
  __shared__ uint32_t s_n[H2C_THREADS / 64];
  // down the rows: a key's, a slot's count in the runs in front
  for (uint64_t k = gid; k < nk; k += nth) {
    uint32_t acc = 0;
    for (uint32_t w = 0; w < (H2C_NBLK); w++) {
      const uint32_t t = F->row_k[(size_t)w * H2C_KEYS_MAX + k];
      F->row_k[(size_t)w * H2C_KEYS_MAX + k] = acc;
      acc += t;
    }
    F->ktot[k] = acc;
  }
  uint32_t nleft = 0;
  for (uint64_t s = gid; s < slots; s += nth) {
    if (neu[s].stream == 0) continue;
    uint32_t acc = 0;
    for (uint32_t w = 0; w < (H2C_NBLK); w++) {
      const uint32_t t = F->row_s[(size_t)w * slots + s];
      F->row_s[(size_t)w * slots + s] = acc;
      acc += t;
    }
    nleft += F->aux[s].left_at != H2C_NONE;
  }
  if (nleft) atomicAdd(&F->nleft, nleft);  // (a count: its order is free)
  // the newly expired: the rank by stream
  const uint32_t nexp = F->nexp < slots / 2u ? F->nexp : slots / 2u;
  for (uint64_t k = gid; k < nexp; k += nth) {
    const uint32_t mine = neu[F->exp_slot[k]].stream;
    uint32_t r = 0;
    for (uint32_t j = 0; j < nexp; j++) r += neu[F->exp_slot[j]].stream < mine;
    F->exp_rank[k] = r;
  }
  // the closes of this run of events
  uint64_t b0, b1;
  h2c_run(C->nev, H2C_BLK, H2C_NBLK, &b0, &b1);
  uint32_t n = 0;
  for (uint64_t j0 = b0; j0 < b1; j0 += H2C_THREADS) {  // (uniform)
    const uint64_t j = j0 + tid;
    uint32_t slot;
    const bool mine = j < b1 && h2c_closes(F, neu, C->ev[j], j, &slot);
    n += (uint32_t)__builtin_popcountll(__ballot(mine));
  }
  if ((tid & 63u) == 0) s_n[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
    for (uint32_t k = 0; k < H2C_THREADS / 64; k++) t += s_n[k];
    F->closes[H2C_BLK] = t;
  }
#elif H2C_STAGE == 7  // k_h2_calls_finish: one workgroup per table
  const uint32_t tid = threadIdx.x;
  __shared__ uint64_t s_wave[H2C_THREADS / 64];
  const uint32_t nm = F->nmethods, nk = nm + 1u;
  const unsigned long long bad = F->bad;
  if (bad != ~0ull) {  // (uniform) the result block alone
    if (tid == 0) {
      for (int k = 0; k < 8; k++) R[k] = 0;
      R[H2C_FLAGS] = H2C_F_BAD_INPUT | (bad & 0xffu) << 8 | (bad >> 8) << 32;
    }
    return;
  }
  // the segments: the scan over the keys' totals (in place: ktot[k] becomes the start of k's segment, ktot[nk] the total)
  uint64_t run = 0;
  for (uint32_t k0 = 0; k0 < nk; k0 += H2C_THREADS) {  // (uniform: the scan's barriers)
    const uint32_t k = k0 + tid;
    const uint32_t v = k < nk ? F->ktot[k] : 0u;
    uint64_t tot;
    const uint64_t x = run + block_excl_scan((uint64_t)v, s_wave, &tot);
    if (k < nk) F->ktot[k] = (uint32_t)x;
    run += tot;
  }
  __syncthreads();
  if (tid != 0) return;
  F->ktot[nk] = (uint32_t)run;  // (= nmsgs)
  const uint64_t orphans = run - F->ktot[nm], dispatched = F->ktot[nm];
  uint64_t wins = 0, closes = 0, bytes = 0;
  for (uint32_t w = 0; w < (H2C_NBLK); w++) wins += F->wins[w], closes += F->closes[w], bytes += F->wg_bytes[w];
  const uint64_t room = F->slots / 2u - F->live, opened = wins < room ? wins : room;
  const uint32_t lost = F->lost | (wins > room ? 1u : 0u);
  const uint64_t nexp = F->nexp, ndone = nexp + closes, live = F->live + opened - F->nleft;
  const bool over = C->disp_cap < C->nmsgs || C->done_cap < ndone;
  R[H2C_OPENED] = opened;
  R[H2C_DISPATCHED] = dispatched;
  R[H2C_ORPHANS] = orphans;
  R[H2C_DONE] = ndone;
  R[H2C_EXPIRED] = nexp;
  R[H2C_LIVE] = live;
  R[H2C_FLAGS] = lost ? H2C_F_LOST : 0u;
  R[H2C_OVERFLOW] = over ? 1u : 0u;
  if (over) return;
  // the commit
  F->go = 1;
  F->emit_tab = 1u - F->cur;
  F->cur = 1u - F->cur;
  F->live = (uint32_t)live;
  F->lost = lost;
  F->serial += opened;
  F->st_steps += 1;
  F->st_opened += opened;
  F->st_msgs += dispatched;
  F->st_bytes += bytes;
  F->st_orphans += orphans;
  F->st_done += ndone;
#elif H2C_STAGE == 8  // k_h2_calls_emit
  if (!F->go) return;  // (uniform) bad input or a cap too small: nothing is written
  const uint32_t tid = threadIdx.x;
  const uint64_t gid = (uint64_t)(H2C_BLK) * H2C_THREADS + tid, nth = (uint64_t)(H2C_NBLK) * H2C_THREADS;
  __shared__ uint64_t s_wave[H2C_THREADS / 64];
  h2c_entry* const neu = F->tab[F->emit_tab];
  const uint32_t slots = F->slots, nm = F->nmethods;
  const uint32_t* const row_s = F->row_s + (size_t)(H2C_BLK) * slots;
  const uint32_t* const row_k = F->row_k + (size_t)(H2C_BLK) * H2C_KEYS_MAX;
  // the segment words, whole
  for (uint64_t k = gid; k < (uint64_t)nm + 2u; k += nth) C->segs[k] = F->ktot[k];
  // the dispatch records of this run
  uint64_t b0, b1;
  h2c_run(C->nmsgs, H2C_BLK, H2C_NBLK, &b0, &b1);
  for (uint64_t i = b0 + tid; i < b1; i += H2C_THREADS) {
    const h2c_msg m = C->msgs[i];
    const h2c_mrec r = C->mrec[i];
    const uint64_t at = (uint64_t)F->ktot[r.key] + row_k[r.key] + r.rank_k;
    h2c_disp o = {m.offset, m.length, 0, m.stream, (uint32_t)i, H2C_NONE, (m.flags & 1u) ? (uint32_t)H2C_COMPRESSED : 0u, 0, 0};
    if (r.key != nm) {
      const h2c_aux a = F->aux[r.slot];
      o.call = neu[r.slot].call;
      o.method = r.key;
      o.seq = a.m0 + row_s[r.slot] + r.rank_s;
      o.word |= (neu[r.slot].word & 0xffu) << 16;
      if (o.seq == 0) o.word |= H2C_FIRST;
      if (a.last == (uint32_t)i + 1u && (a.left_at & a.rc_at) != H2C_NONE) o.word |= H2C_LAST;
    } else {
      o.word |= r.rank_s << 8;
      if (r.slot != H2C_NONE) o.call = neu[r.slot].call, o.word |= (neu[r.slot].word & 0xffu) << 16;
    }
    if (at < C->disp_cap) C->disp[at] = o;  // (at < nmsgs <= disp_cap)
  }
  // the done list: the deadlines by stream ...
  const uint32_t nexp = F->nexp < slots / 2u ? F->nexp : slots / 2u;
  for (uint64_t k = gid; k < nexp; k += nth) {
    const uint32_t s = F->exp_slot[k];
    const h2c_entry e = neu[s];
    // (an expired entry is dispatched nothing: its count and bytes are those it came with)
    const h2c_done o = {e.call, e.bytes, e.stream, e.method, e.messages, H2C_DEADLINE | ((e.word & H2C_EF_READS_CLOSED) ? 1u << 8 : 0u)};
    if (F->exp_rank[k] < C->done_cap) C->done[F->exp_rank[k]] = o;
  }
  // ... then the closes of this run of events, in event order
  uint64_t run = nexp;
  for (uint32_t w = 0; w < (H2C_BLK); w++) run += F->closes[w];
  h2c_run(C->nev, H2C_BLK, H2C_NBLK, &b0, &b1);
  for (uint64_t j0 = b0; j0 < b1; j0 += H2C_THREADS) {  // (uniform: the scan's barriers)
    const uint64_t j = j0 + tid;
    uint32_t s = 0;
    grdma_h2_event ev = {0, 0, 0, 0, 0, 0};
    if (j < b1) ev = C->ev[j];
    const bool mine = j < b1 && h2c_closes(F, neu, ev, j, &s);
    uint64_t tot;
    const uint64_t x = run + block_excl_scan(mine ? 1ull : 0ull, s_wave, &tot);
    if (mine && x < C->done_cap) {
      const h2c_aux a = F->aux[s];
      uint32_t word = H2C_READS_CLOSED;
      if (ev.a) word = H2C_LEFT | (((neu[s].word & H2C_EF_READS_CLOSED) || a.rc_at < a.left_at) ? 1u << 8 : 0u);
      const h2c_done o = {neu[s].call, neu[s].bytes, neu[s].stream, neu[s].method, a.m0 + a.nstep, word};
      C->done[x] = o;
    }
    run += tot;
  }
  // the entries made final: what the step's closes add goes into `fin`, which no stage of this step reads, and the count
  // of an entry another workgroup may still read (a DEADLINE record's) is an expired entry's, which does not change
  for (uint64_t s = gid; s < slots; s += nth) {
    if (neu[s].stream == 0) continue;
    const h2c_aux a = F->aux[s];
    neu[s].messages = a.m0 + a.nstep;
    neu[s].fin = (a.rc_at != H2C_NONE ? (uint32_t)H2C_EF_READS_CLOSED : 0u) | (a.left_at != H2C_NONE ? (uint32_t)H2C_EF_DEAD : 0u);
  }
#endif
