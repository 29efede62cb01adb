// The bodies of the send windows' stages as source text, included by the single-transport kernels (k_h2_sw_*: the grid is
// the call's, H2SW_BLK = blockIdx.x, H2SW_NBLK = gridDim.x) and by the many-link kernels (k_h2_links_sw_*: a link's share
// of the grid, or one workgroup per link), csrc/grdma_h2_sw.h.  H2SW_STAGE selects the stage; every stage expects
// `h2sw_dev* F` (the emit: `const h2sw_dev* F`) and, for the take and the finish, `const h2sw_call* call` in scope, as
// the single-transport kernels' parameters are.  Stage 5 is the emit of ONE transport: k_h2_links_sw_emit spreads the
// pieces of all links over one grid and shares h2sw_emit_piece with it, not this text.
// (Source text rather than device functions, as csrc/grdma_h2_fc_stage.inc: with included text tools/h2_isa_compare.py
// reports the five single-transport kernels `same`.)
#if H2SW_STAGE == 1  // k_h2_sw_clear
  const uint64_t t0 = (uint64_t)H2SW_BLK * H2SW_THREADS + threadIdx.x, step = (uint64_t)H2SW_NBLK * H2SW_THREADS;
  h2sw_slot* neu = F->tabs[F->cur ^ 1u];
  const h2sw_slot empty = {0, H2SW_NONE, 0, 0, 0, 0};
  for (uint64_t s = t0; s <= F->tab_mask; s += step) neu[s] = empty;
  if (t0 == 0) {  // (the first thread of the grid, or of the link's share)
    F->c_conn = 0;
    F->c_first = ~0ull;
    F->c_iws = F->c_mfs = 0;
    F->c_applied = F->c_nset = F->c_bad_inc = F->c_bad_set = F->c_full = 0;
    F->c_conn_first = H2SW_NONE;
    F->carry_out.type = 0;
  }
#elif H2SW_STAGE == 2  // k_h2_sw_take
  if (!h2sw_taken(call)) return;  // (uniform) nothing is taken in
  const uint64_t n = call->res->nevents;
  const uint64_t t0 = (uint64_t)H2SW_BLK * H2SW_THREADS + threadIdx.x, step = (uint64_t)H2SW_NBLK * H2SW_THREADS;
  const uint32_t m = F->tab_mask;
  const h2sw_slot* old = F->tabs[F->cur];
  h2sw_slot* neu = F->tabs[F->cur ^ 1u];
  // the entries of the streams the map holds behind the call
  for (uint64_t s = t0; s <= m; s += step) {
    const h2sw_slot e = old[s];
    if (e.key == 0 || tab_find(F->gp->tab, F->gp->tab_mask, e.key) < 0) continue;
    const uint32_t t = h2sw_claim(neu, m, e.key);
    if (t == H2SW_NONE) atomicExch(&F->c_full, 1u);
    else atomicAdd(reinterpret_cast<unsigned long long*>(&neu[t].delta), (unsigned long long)e.delta);
  }
  // the carried frame goes on over the PAYLOAD events in front of the first FRAME event (position 0): the first thread
  // of the grid, or of the link's share
  if (t0 == 0 && F->carry.type != 0 && !call->skipped) h2sw_walk(F, call, neu, F->carry, 0, n, 0);
  // a frame per thread (position: its event index + 1)
  for (uint64_t i = t0; i < n; i += step) {
    const grdma_h2_event e = call->ev[i];
    if (e.kind != EV_FRAME || (e.b >> 8) != 0) continue;
    if (e.a != FT_WINDOW_UPDATE && !(e.a == FT_SETTINGS && !(e.b & 1u))) continue;
    const h2sw_frame f = {e.a, e.c, 0, 0, 0, 0, 0};
    h2sw_walk(F, call, neu, f, i + 1, n, (uint32_t)i + 1u);
  }
#elif H2SW_STAGE == 3  // k_h2_sw_finish
  __shared__ uint64_t s_wave[H2SW_THREADS / 64];
  __shared__ unsigned long long s_first;
  __shared__ uint32_t s_over;
  const uint32_t tid = threadIdx.x;
  const bool lost = h2sw_lost(call), taken = h2sw_taken(call);
  const bool full = taken && F->c_full != 0;  // (cannot be: the map holds at most half as many streams as the table has slots)
  const bool apply = taken && !full;
  const uint32_t iws = (apply && F->c_iws) ? (uint32_t)F->c_iws : F->iws;
  if (tid == 0) {
    s_first = F->c_first;
    s_over = 0;
  }
  __syncthreads();
  // ---- per slot of the table that is current behind the call: the credit, the clamp; how many entries live
  h2sw_slot* T = F->tabs[apply ? (F->cur ^ 1u) : F->cur];
  uint64_t live = 0, added = 0;
  for (uint32_t t = tid; t <= F->tab_mask; t += H2SW_THREADS) {
    h2sw_slot sl = T[t];
    if (sl.key == 0) continue;
    live++;
    if (apply && sl.credit) {
      const long long old = (long long)iws + sl.delta;
      long long nw = old + (long long)sl.credit;
      if (nw > H2SW_MAXW) {
        nw = old > H2SW_MAXW ? old : H2SW_MAXW;
        atomicAdd(&s_over, 1u);
        atomicMin(&s_first, ((unsigned long long)sl.first << 32) | sl.key);
      }
      added += (uint64_t)(nw - old);
      sl.delta = nw - (long long)iws;
    }
    if (apply) {
      sl.credit = 0;
      sl.first = H2SW_NONE;
      T[t] = sl;
    }
  }
  uint64_t n_live, n_added;
  block_excl_scan(live, s_wave, &n_live);
  block_excl_scan(added, s_wave, &n_added);
  if (tid != 0) return;
  if (call->skipped || lost || full) F->lost = 1;
  if (call->skipped || lost) F->carry.type = 0;  // (its frame's end was not seen)
  F->st_intakes++;
  for (int k = 0; k < 8; k++) F->res[k] = 0;
  F->res[H2SW_I_LIVE] = n_live;
  F->res[H2SW_I_VIOLATIONS] = F->lost ? H2SW_V_LOST : 0;
  if (lost || full) F->res[H2SW_I_OVERFLOW] = 2;
  if (!apply) return;
  // ---- the connection, the settings, the carry
  uint64_t viol = 0, conn_added = 0, nviol = F->c_bad_inc + F->c_bad_set + s_over;
  unsigned long long first = s_first;
  if (F->c_conn) {
    const long long old = F->conn;
    long long nw = old + (long long)F->c_conn;  // (increments only add inside an intake: judging the call's sum is exact)
    if (nw > H2SW_MAXW) {
      nw = H2SW_MAXW;
      nviol++;
      viol |= H2SW_V_WINDOW;
      const unsigned long long o = (unsigned long long)F->c_conn_first << 32;
      if (o < first) first = o;
    }
    conn_added = (uint64_t)(nw - old);
    F->conn = nw;
  }
  if (F->c_iws) F->iws = (uint32_t)F->c_iws;
  if (F->c_mfs) F->pmf = (uint32_t)F->c_mfs;
  F->carry = F->carry_out;
  F->cur ^= 1u;
  viol |= (F->c_bad_inc ? H2SW_V_INCREMENT : 0) | (F->c_bad_set ? H2SW_V_SETTINGS : 0) | (s_over ? H2SW_V_WINDOW : 0);
  F->res[H2SW_I_UPDATES] = F->c_applied;
  F->res[H2SW_I_CONN] = conn_added;
  F->res[H2SW_I_STREAMS] = n_added;
  F->res[H2SW_I_SETTINGS] = F->c_nset;
  F->res[H2SW_I_VIOLATIONS] |= viol;
  F->res[H2SW_I_FIRST] = first == ~0ull ? 0 : (uint32_t)first;
  F->st_updates += F->c_applied;
  F->st_settings += F->c_nset;
  F->st_violations += nviol;
#elif H2SW_STAGE == 4  // k_h2_sw_plan
  __shared__ uint64_t s_wave[H2SW_PLAN_THREADS / 64];
  // the tiles' aggregates of a block of messages: per wave the streams of its tile with their remaining bytes
  __shared__ uint64_t s_agg[H2SW_PLAN_THREADS / 64][64];
  __shared__ uint32_t s_key[H2SW_PLAN_THREADS / 64][64];
  __shared__ uint32_t s_cnt[H2SW_PLAN_THREADS / 64];
  __shared__ uint32_t s_stall[3];
  const uint32_t tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  h2sw_slot* T = F->tabs[F->cur];
  const uint32_t m = F->tab_mask;
  const uint64_t n = F->nmsgs;
  const uint32_t mf = (uint32_t)(F->max_frame < F->pmf ? F->max_frame : F->pmf);
  const long long C = F->conn, iws = (long long)F->iws;
  const grdma_h2_msg_dev* msgs = F->msgs;
  h2sw_piece* pieces = F->pieces;
  if (tid < 3) s_stall[tid] = 0;
  __syncthreads();
  // ---- the grant, the granted pieces compacted in table order
  uint64_t base_a = 0, kept = 0, granted = 0, done = 0;
  for (uint64_t m0 = 0; m0 < n; m0 += H2SW_PLAN_THREADS) {
    const uint64_t i = m0 + tid;
    grdma_h2_msg_dev msg{nullptr, 0, 0, 0};
    uint64_t p = 0, r = 0;
    uint32_t slot = H2SW_NONE;
    if (i < n) {
      msg = msgs[i];
      p = F->prog_in[i];
      r = 5 + msg.len - p;  // (the host has refused r == 0)
    }
    // Per distinct stream of my wave's tile (ballot, readlane, a masked scan, as k_h2_asm_tiles): ONE lane looks the
    // stream up and claims its slot -- a stream the map does not hold gets nothing; one it holds has an entry from
    // here on, delta 0 until it moves -- and the remaining bytes of the tile's earlier messages of the stream are summed.
    uint64_t x = 0, agg = 0;
    bool closes = false;  // the tile's last message of its stream
    uint64_t rem = __ballot(msg.stream_id != 0);
    while (rem) {
      const int first = __builtin_ctzll(rem);
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)msg.stream_id, first);
      const bool mem = msg.stream_id == k;
      const uint64_t mm = __ballot(mem);
      uint32_t sk = H2SW_NONE;
      if (lane == first && tab_find(F->gp->tab, F->gp->tab_mask, k) >= 0) sk = h2sw_claim(T, m, k);
      sk = (uint32_t)__builtin_amdgcn_readlane((int)sk, first);
      if (sk != H2SW_NONE) {  // (uniform)
        const uint64_t incl = wave_incl_scan(mem ? r : 0, lane);
        if (mem) {
          slot = sk;
          x = incl - r;
          if (lane == 63 - __builtin_clzll(mm)) {
            closes = true;
            agg = incl;
          }
        }
      }
      rem &= ~mm;
    }
    const uint32_t key = slot != H2SW_NONE ? msg.stream_id : 0;
    if (i < n) F->slot_of[i] = closes ? (slot | 0x80000000u) : slot;  // (bit 31: the one that settles the tile's sum below)
    // the stream's window, and the remaining bytes of its messages in the blocks in front (the slot carries them)
    long long delta = 0;
    uint64_t c = 0;
    if (key) {
      delta = T[slot].delta;
      c = T[slot].run;
    }
    // ... and in the earlier tiles of the block: every tile lists its streams' sums in LDS
    const uint64_t cm = __ballot(closes);
    if (closes) {
      const uint32_t at = (uint32_t)__builtin_popcountll(cm & ((1ull << lane) - 1ull));
      s_key[wave][at] = key;
      s_agg[wave][at] = agg;
    }
    if (lane == 0) s_cnt[wave] = (uint32_t)__builtin_popcountll(cm);
    __syncthreads();
    if (key) {
      for (int w = 0; w < wave; w++) {
        const uint32_t cnt = s_cnt[w];
        for (uint32_t j = 0; j < cnt; j++)
          if (s_key[w][j] == key) c += s_agg[w][j];
      }
      if (closes) {  // the block's last message of the stream hands the sum to the next block
        bool later = false;
        for (int w = wave + 1; w < H2SW_PLAN_THREADS / 64; w++) {
          const uint32_t cnt = s_cnt[w];
          for (uint32_t j = 0; j < cnt; j++) later = later || s_key[w][j] == key;
        }
        if (!later) T[slot].run = c + agg;
      }
    }
    uint64_t a = 0;
    if (key) {
      const long long room = iws + delta - (long long)(c + x);
      a = room <= 0 ? 0 : ((uint64_t)room < r ? (uint64_t)room : r);
    }
    uint64_t tot_a;
    const uint64_t pre = base_a + h2sw_block_scan(a, s_wave, &tot_a);
    base_a += tot_a;
    const long long croom = C - (long long)pre;
    const uint64_t g = croom <= 0 ? 0 : ((uint64_t)croom < a ? (uint64_t)croom : a);
    if (i < n) {
      if (!key) atomicAdd(&s_stall[2], 1u);
      else if (a < r) atomicAdd(&s_stall[1], 1u);
      if (g < a) atomicAdd(&s_stall[0], 1u);
      F->prog_out[i] = p + g;
    }
    // what the tile grants per stream, added to the stream's slot by the tile's last message of the stream
    uint64_t rem_g = __ballot(key != 0);
    while (rem_g) {
      const int first = __builtin_ctzll(rem_g);
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
      const bool mem = key == k;
      const uint64_t mm = __ballot(mem);
      const uint64_t incl = wave_incl_scan(mem ? g : 0, lane);
      if (mem && closes && incl) atomicAdd(&T[slot].sent, (unsigned long long)incl);
      rem_g &= ~mm;
    }
    uint64_t tot;
    const uint64_t xk = h2sw_block_scan(g ? 1 : 0, s_wave, &tot);
    if (g) pieces[kept + xk] = h2sw_piece{msg.payload, msg.len, msg.stream_id, msg.flags, p, g};
    kept += tot;
    h2sw_block_scan(g, s_wave, &tot);
    granted += tot;
    h2sw_block_scan((i < n && g == r) ? 1 : 0, s_wave, &tot);
    done += tot;
  }
  __syncthreads();  // the piece table is complete: sizes look at a piece's neighbours
  // ---- sizes and positions over the pieces (the loop of k_h2_frame_index)
  uint64_t base_sl = 0, base_hdr = 0, base_wire = 0;
  for (uint64_t k0 = 0; k0 < kept; k0 += H2SW_PLAN_THREADS) {
    const uint64_t k = k0 + tid;
    uint64_t n_sl = 0, n_hdr = 0, n_wire = 0;
    uint32_t mode = 0;
    if (k < kept) h2sw_piece_size(pieces, k, mf, &n_sl, &n_hdr, &n_wire, &mode);
    uint64_t tot_sl, tot_hdr, tot_wire;
    const uint64_t x_sl = h2sw_block_scan(n_sl, s_wave, &tot_sl);
    const uint64_t x_hdr = h2sw_block_scan(n_hdr, s_wave, &tot_hdr);
    h2sw_block_scan(n_wire, s_wave, &tot_wire);
    if (k < kept) {
      grdma_h2_msg_pos q;
      q.sl = base_sl + x_sl;
      q.hdr = base_hdr + x_hdr;
      q.mode = mode;
      q.pad = 0;
      F->pos[k] = q;
    }
    base_sl += tot_sl;
    base_hdr += tot_hdr;
    base_wire += tot_wire;
  }
  const bool over = base_sl > F->cap || base_hdr > F->hdr_cap;  // (uniform: the totals are every thread's)
  // ---- the windows move only when the bytes go out; the slots' scratch words go back to 0 either way.  Per tile and
  // stream (the thread that added the tile's sum: its own word of the first pass), no sweep over the table: the first
  // one to exchange a stream's sum for 0 moves the stream's window by it.
  for (uint64_t i = tid; i < n; i += H2SW_PLAN_THREADS) {
    const uint32_t v = F->slot_of[i];
    if (v == H2SW_NONE || !(v >> 31)) continue;
    const uint32_t slot = v & 0x7fffffffu;
    T[slot].run = 0;
    const unsigned long long sent = atomicExch(&T[slot].sent, 0ull);
    if (!over && sent) atomicAdd(reinterpret_cast<unsigned long long*>(&T[slot].delta), 0ull - sent);
  }
  if (tid == 0) {
    if (!over) {
      F->conn = C - (long long)granted;
      F->st_sent += granted;
    }
    F->st_frame_calls++;
    F->npieces = kept;
    F->fres[H2SW_F_DONE] = over ? 0 : done;
    F->fres[H2SW_F_HELD] = over ? n : n - done;
    F->fres[H2SW_F_SLICES] = base_sl;
    F->fres[H2SW_F_HDR] = base_hdr;
    F->fres[H2SW_F_WIRE] = base_wire;
    F->fres[H2SW_F_GRANTED] = over ? 0 : granted;
    F->fres[H2SW_F_STALL] = (s_stall[0] ? H2SW_STALL_CONN : 0) | (s_stall[1] ? H2SW_STALL_STREAM : 0) | (s_stall[2] ? H2SW_STALL_UNKNOWN : 0);
    F->fres[H2SW_F_OVERFLOW] = over ? 1 : 0;
  }
#elif H2SW_STAGE == 5  // k_h2_sw_emit
  if (F->fres[H2SW_F_OVERFLOW]) return;  // (nothing half-written)
  const uint64_t n = F->npieces;
  const int lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (H2_EMIT_THREADS / 64);
  const h2sw_piece* pieces = F->pieces;
  const grdma_h2_msg_pos* pos = F->pos;
  const uint32_t mf = (uint32_t)(F->max_frame < F->pmf ? F->max_frame : F->pmf);
  grdma_sge* out = F->out;
  uint8_t* hdr = F->hdr;
  const uint64_t cap = F->cap, hdr_cap = F->hdr_cap;
  for (uint64_t k = (uint64_t)blockIdx.x * (H2_EMIT_THREADS / 64) + (threadIdx.x >> 6); k < n; k += waves)
    h2sw_emit_piece(pieces, k, n, mf, out, cap, hdr, hdr_cap, pos[k], lane);
#else
#error "H2SW_STAGE: 1 clear, 2 take, 3 finish, 4 plan, 5 emit"
#endif
