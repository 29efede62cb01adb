// The bodies of the assembler's stages as source text, included by the single-transport kernels (k_h2_asm_*: the
// grid is the call's, H2A_BLK = blockIdx.x, H2A_NBLK = gridDim.x) and by the many-link kernels (k_h2_asm_*_links: a
// link's share of the grid, or one workgroup per link), csrc/grdma_h2_asm.h.  H2A_STAGE selects the stage; every stage
// expects `h2a_dev* A` and `const h2a_call* call` in scope, as the single-transport kernels' parameters are.
// (Source text rather than device functions: csrc/grdma_h2_frame_group.inc records that a function is simplified on its
// own before it is inlined and that the kernel it was taken from then came out as other bytes; with included text
// tools/h2_isa_compare.py reports the seven single-transport kernels `same`.)
#if H2A_STAGE == 1  // k_h2_asm_tiles
  const grdma_h2_deframe_result* res = call->res;
  if (res->overflow || res->nevents > call->ev_cap || res->nevents > A->scratch_ev) return;
  const uint64_t n = res->nevents;
  const int lane = threadIdx.x & 63;
  const uint64_t ntiles = (n + 63) / 64;
  const uint64_t waves = (uint64_t)H2A_NBLK * (H2A_THREADS / 64);
  for (uint64_t t = H2A_BLK * (H2A_THREADS / 64) + (threadIdx.x >> 6); t < ntiles; t += waves) {
    const uint64_t i = t * 64 + lane;
    grdma_h2_event e{0, 0, 0, 0, 0, 0};
    if (i < n) e = call->ev[i];
    uint32_t key;
    h2a_el el;
    h2a_elem_of(e, &key, &el, (uint32_t)i);
    const uint64_t sz = h2a_size_of(A, e);
    const uint64_t bsz = wave_incl_scan(sz, lane);
    const uint64_t bm = __ballot(e.kind == 3 && i < n);
    uint64_t rem = __ballot(key != 0);
    uint32_t r = 0;
    while (rem) {
      const int first = __builtin_ctzll(rem);
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
      const bool mem = key == k;
      const uint64_t mm = __ballot(mem);
      const h2a_el v = h2a_wave_scan(mem ? el : h2a_el{0, 0, 0}, lane);
      const int last = 63 - __builtin_clzll(mm);
      if (lane == last) A->keys[t * 64 + r] = h2a_key{k, v.kind, v.idx, 0, v.bytes, 0};
      rem &= ~mm;
      r++;
    }
    if (lane == 63) {
      h2a_tile& T = A->tiles[t];
      T.nkeys = r;
      T.nbeg = (uint32_t)__builtin_popcountll(bm);
      T.bsz = bsz;
      T.nrep = 0;
    }
  }
#elif H2A_STAGE == 2  // k_h2_asm_carry
  __shared__ uint64_t ws[H2A_ONE_THREADS / 64];
  __shared__ uint64_t s_found, s_c;
  __shared__ uint32_t hkey[H2A_LDS_KEYS], hkind[H2A_LDS_KEYS], hidx[H2A_LDS_KEYS];
  __shared__ uint64_t hbytes[H2A_LDS_KEYS];
  const int tid = threadIdx.x, lane = tid & 63;
  const grdma_h2_deframe_result* res = call->res;
  const bool skip = res->overflow || res->nevents > call->ev_cap || res->nevents > A->scratch_ev;
  if (call->release_all && tid < 64) h2a_release_wave(A, 0, true, lane);
  __syncthreads();
  if (skip) {
    if (tid == 0) {
      A->skip = 1;
      A->n = 0;
    }
    return;
  }
  const uint64_t n = res->nevents;
  const uint64_t ntiles = (n + 63) / 64;
  // tile prefixes: MSG_BEGIN ordinals, granule bytes, aggregate slots
  uint64_t carry_beg = 0, carry_sz = 0, carry_key = 0;
  for (uint64_t t0 = 0; t0 < ntiles; t0 += H2A_ONE_THREADS) {
    const uint64_t t = t0 + tid;
    h2a_tile T{};
    if (t < ntiles) T = A->tiles[t];
    uint64_t tb, ts, tk;
    const uint64_t eb = h2a_block_scan(t < ntiles ? T.nbeg : 0, ws, &tb);
    const uint64_t es = h2a_block_scan(t < ntiles ? T.bsz : 0, ws, &ts);
    const uint64_t ek = h2a_block_scan(t < ntiles ? T.nkeys : 0, ws, &tk);
    if (t < ntiles) {
      A->tiles[t].beg_base = carry_beg + eb;
      A->tiles[t].sz_base = carry_sz + es;
      A->tiles[t].key_base = carry_key + ek;
      for (uint32_t r = 0; r < T.nkeys; r++) A->comp[carry_key + ek + r] = (uint32_t)(t * 64 + r);
    }
    carry_beg += tb;
    carry_sz += ts;
    carry_key += tk;
  }
  const uint64_t nbeg = carry_beg, nkeys = carry_key;
  __syncthreads();
  // the allocation plan: the first MSG_BEGIN that does not fit in front of the arena's end wraps to 0; the first one that
  // does not fit in the free space, or would hold more than max_pending records, and every later one, get NO_SPACE
  const uint64_t AB = A->arena_bytes, vh = A->vh, vt = A->vt, hp = vh % AB;
  const uint64_t live = A->rec_head - A->rec_tail;
  uint64_t wrap_ord = ~0ull, c_wrap = 0, waste = 0;
  {
    if (tid == 0) s_found = ~0ull;
    __syncthreads();
    for (uint64_t t = tid; t < ntiles; t += H2A_ONE_THREADS) {
      const h2a_tile& T = A->tiles[t];
      if (T.bsz && hp + T.sz_base + T.bsz > AB) atomicMin((unsigned long long*)&s_found, (unsigned long long)t);
    }
    __syncthreads();
    const uint64_t ft = s_found;
    if (ft != ~0ull && tid < 64) {
      uint64_t c = 0;
      const uint64_t o = h2a_first_in_tile(A, call, ft, n, [&](uint64_t cc, uint64_t s) { return s && hp + cc + s > AB; }, &c, lane);
      if (tid == 0) {
        s_found = o;
        s_c = c;
      }
    }
    __syncthreads();
    if (ft != ~0ull) {
      wrap_ord = s_found;
      c_wrap = s_c;
      waste = AB - hp - c_wrap;
    }
    __syncthreads();
  }
  uint64_t cutoff = nbeg;
  {
    // ends are monotone in the ordinal: the end of a tile's last sized message bounds them all
    if (tid == 0) s_found = ~0ull;
    __syncthreads();
    for (uint64_t t = tid; t < ntiles; t += H2A_ONE_THREADS) {
      const h2a_tile& T = A->tiles[t];
      if (!T.bsz) continue;
      const uint64_t cend = T.sz_base + T.bsz;
      const bool after = wrap_ord != ~0ull && cend > c_wrap;  // the tile's last sized message is at or after the wrap
      const uint64_t end = vh + cend + (after ? waste : 0);
      if (end - vt > AB) atomicMin((unsigned long long*)&s_found, (unsigned long long)t);
    }
    __syncthreads();
    const uint64_t gt = s_found;
    __syncthreads();
    if (gt != ~0ull && tid < 64) {
      uint64_t c = 0;
      // (a sized message is at or after the wrap exactly when its prefix is: those in front end at or before c_wrap)
      const uint64_t o = h2a_first_in_tile(A, call, gt, n, [&](uint64_t cc, uint64_t s) {
        return s && vh + cc + s + ((wrap_ord != ~0ull && cc >= c_wrap) ? waste : 0) - vt > AB;
      }, &c, lane);
      if (tid == 0) s_found = o;
    }
    __syncthreads();
    if (gt != ~0ull && s_found < cutoff) cutoff = s_found;
    const uint64_t room = A->max_pending > live ? A->max_pending - live : 0;
    if (room < cutoff) cutoff = room;
  }
  if (tid == 0) {
    A->skip = 0;
    A->n = n;
    A->wrap_ord = wrap_ord;
    A->c_wrap = c_wrap;
    A->waste = waste;
    A->cutoff = cutoff;
    A->seq_base = A->seq;
    A->rec_base = A->rec_head;
    A->vh0 = vh;
  }
  // the keyed scan over the tile aggregates: wave 0, 64 aggregates per step, running state per stream in LDS
  for (uint32_t s = tid; s < H2A_LDS_KEYS; s += H2A_ONE_THREADS) hkey[s] = 0;
  __syncthreads();
  if (tid < 64) {
    bool full = false;
    // distinct streams so far.  Counted from a ballot, so every lane holds the same number: a counter in LDS that only
    // the inserting lane bumps is, to the compiler, a value no other lane's code changed -- it may keep it in a
    // register, and the lanes then disagree about `full`
    uint32_t cnt = 0;
    // software pipeline: the aggregates of the next step and the slots of the one after are in flight while this one
    // is scanned (the loads are not used before the next iteration)
    uint32_t slot = 0, slot1 = 0;
    h2a_key kv{0, 0, 0, 0, 0, 0};
    if ((uint64_t)lane < nkeys) {
      slot = A->comp[lane];
      kv = A->keys[slot];
    }
    if (64 + (uint64_t)lane < nkeys) slot1 = A->comp[64 + lane];
    for (uint64_t x0 = 0; x0 < nkeys && !full; x0 += 64) {
      const uint64_t x = x0 + lane;
      h2a_key kv1{0, 0, 0, 0, 0, 0};
      uint32_t slot2 = 0;
      if (x + 64 < nkeys) kv1 = A->keys[slot1];
      if (x + 128 < nkeys) slot2 = A->comp[x + 128];
      const h2a_el el{kv.kind, kv.idx, kv.bytes};
      uint64_t rem = __ballot(x < nkeys);
      while (rem) {
        const int first = __builtin_ctzll(rem);
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)kv.key, first);
        const bool mem = x < nkeys && kv.key == k;
        const uint64_t mm = __ballot(mem);
        // the stream's running state (first lane: find or insert)
        uint32_t hs = 0;
        bool inserted = false;
        if (lane == first) {
          hs = (k >> 1) & (H2A_LDS_KEYS - 1);
          while (hkey[hs] != 0 && hkey[hs] != k) hs = (hs + 1) & (H2A_LDS_KEYS - 1);
          if (hkey[hs] == 0) {
            hkey[hs] = k;
            hkind[hs] = 0;
            hidx[hs] = 0;
            hbytes[hs] = 0;
            inserted = true;
          }
        }
        cnt += __ballot(inserted) ? 1u : 0u;
        hs = (uint32_t)__builtin_amdgcn_readlane((int)hs, first);
        const h2a_el base{hkind[hs], hidx[hs], hbytes[hs]};
        const h2a_el inc = h2a_wave_scan(mem ? el : h2a_el{0, 0, 0}, lane);
        h2a_el ex;
        ex.kind = __shfl_up(inc.kind, 1, 64);
        ex.idx = __shfl_up(inc.idx, 1, 64);
        ex.bytes = __shfl_up(inc.bytes, 1, 64);
        if (lane == 0) ex = h2a_el{0, 0, 0};
        if (mem) {
          const h2a_el out = h2a_combine(base, ex);
          A->keys[slot] = h2a_key{k, out.kind, out.idx, 0, out.bytes, 0};
        }
        const int last = 63 - __builtin_clzll(mm);
        const h2a_el tot = h2a_combine(base, h2a_el{
            (uint32_t)__builtin_amdgcn_readlane((int)inc.kind, last), (uint32_t)__builtin_amdgcn_readlane((int)inc.idx, last),
            ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(inc.bytes >> 32), last) << 32) |
                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)inc.bytes, last)});
        if (lane == first) {
          hkind[hs] = tot.kind;
          hidx[hs] = tot.idx;
          hbytes[hs] = tot.bytes;
        }
        rem &= ~mm;
      }
      full = cnt > H2A_LDS_KEYS / 4 * 3;
      slot = slot1;
      kv = kv1;
      slot1 = slot2;
    }
    if (full) {
      // more distinct streams than the plan holds: the call fails and nothing is assembled -- no descriptor, no byte, ring
      // and seq as they were.  The deframer has consumed the call's bytes all the same, so a message a stream carried
      // into the call can never be completed: it is dropped here (entry cleared, record freed) and never reported.
      for (uint32_t s = lane; s <= A->tab_mask; s += 64) {
        const h2a_carry c = A->tab[s];
        if (!c.stream_id) continue;
        if (c.rec != ~0ull) A->recs[c.rec % A->max_pending].freed = 1;
        A->tab[s].stream_id = 0;
      }
      if (lane == 0) A->skip = 2;
    } else {
      // the final state of every stream the call touched, for k_h2_asm_finish
      uint64_t nf = 0;
      for (uint32_t s0 = 0; s0 < H2A_LDS_KEYS; s0 += 64) {
        const uint32_t s = s0 + lane;
        const bool used = hkey[s] != 0;
        const uint64_t um = __ballot(used);
        if (used) {
          const uint64_t at = nf + (uint64_t)__builtin_popcountll(um & ((1ull << lane) - 1));
          A->fin[at] = h2a_key{hkey[s], hkind[s], hidx[s], 0, hbytes[s], 0};
        }
        nf += (uint64_t)__builtin_popcountll(um);
      }
      if (lane == 0) {
        A->nfin = nf;
        A->seq += nbeg;  // (only a call that is assembled numbers its messages)
      }
    }
  }
#elif H2A_STAGE == 3  // k_h2_asm_begin
  if (A->skip) return;
  const uint64_t n = A->n;
  const int lane = threadIdx.x & 63;
  const uint64_t ntiles = (n + 63) / 64;
  const uint64_t waves = (uint64_t)H2A_NBLK * (H2A_THREADS / 64);
  const uint64_t AB = A->arena_bytes;
  for (uint64_t t = H2A_BLK * (H2A_THREADS / 64) + (threadIdx.x >> 6); t < ntiles; t += waves) {
    const uint64_t i = t * 64 + lane;
    grdma_h2_event e{0, 0, 0, 0, 0, 0};
    if (i < n) e = call->ev[i];
    const uint64_t sz = h2a_size_of(A, e);
    const uint64_t c = A->tiles[t].sz_base + wave_incl_scan(sz, lane) - sz;
    const bool beg = e.kind == 3 && i < n;
    const uint64_t bm = __ballot(beg);
    if (!beg) continue;
    const uint64_t k = A->tiles[t].beg_base + (uint64_t)__builtin_popcountll(bm & ((1ull << lane) - 1));
    h2a_msg m;
    m.length = e.b;
    m.seq = A->seq_base + k;
    m.stream = e.c;
    m.flags = e.a & 1;
    m.pad = 0;
    m.offset = 0;
    m.rec = ~0ull;
    if (k >= A->cutoff) {
      m.status = GRDMA_H2_MSG_NO_SPACE;
    } else {
      m.status = (A->max_msg && e.b > A->max_msg) ? GRDMA_H2_MSG_TOO_LARGE : GRDMA_H2_MSG_OK;
      m.rec = A->rec_base + k;
      const uint64_t v = h2a_start(A, k, c);  // (a message of no size is never the one that wraps)
      if (sz) m.offset = v % AB;
      A->recs[m.rec % A->max_pending] = h2a_rec{v, v + sz, ~0ull, 0};
    }
    A->msgs[i] = m;
  }
#elif H2A_STAGE == 4  // k_h2_asm_bytes
  if (A->skip) return;
  const uint64_t n = A->n;
  const int lane = threadIdx.x & 63;
  const uint64_t ntiles = (n + 63) / 64;
  const uint64_t waves = (uint64_t)H2A_NBLK * (H2A_THREADS / 64);
  for (uint64_t t = H2A_BLK * (H2A_THREADS / 64) + (threadIdx.x >> 6); t < ntiles; t += waves) {
    const uint64_t i = t * 64 + lane;
    grdma_h2_event e{0, 0, 0, 0, 0, 0};
    if (i < n) e = call->ev[i];
    uint32_t key;
    h2a_el el;
    h2a_elem_of(e, &key, &el, (uint32_t)i);
    // this event's exclusive state: the tile aggregate's prefix (k_h2_asm_carry) + the wave's own scan
    h2a_el st{0, 0, 0};
    uint64_t rem = __ballot(key != 0);
    uint32_t r = 0;
    while (rem) {
      const int first = __builtin_ctzll(rem);
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
      const bool mem = key == k;
      const uint64_t mm = __ballot(mem);
      const h2a_el inc = h2a_wave_scan(mem ? el : h2a_el{0, 0, 0}, lane);
      h2a_el ex;
      ex.kind = __shfl_up(inc.kind, 1, 64);
      ex.idx = __shfl_up(inc.idx, 1, 64);
      ex.bytes = __shfl_up(inc.bytes, 1, 64);
      if (lane == 0) ex = h2a_el{0, 0, 0};
      if (mem) {
        const h2a_key& b = A->keys[t * 64 + r];
        st = h2a_combine(h2a_el{b.kind, b.idx, b.bytes}, ex);
      }
      rem &= ~mm;
      r++;
    }
    h2a_piece pc{nullptr, nullptr, 0, 0};
    grdma_h2_rx_msg d{0, 0, 0, 0, 0, 0, 0};
    if (key && e.kind != 3 && st.kind != H2A_SHUT) {
      // the message: begun in this call, or carried in
      bool have = false;
      h2a_msg m;
      uint64_t fill = st.bytes;
      if (st.kind == H2A_OPEN) {
        m = A->msgs[st.idx];
        have = true;
      } else {
        const uint64_t s = h2a_tab_find(A, key);
        if (s != ~0ull) {
          const h2a_carry& cr = A->tab[s];
          m = h2a_msg{cr.offset, cr.length, cr.seq, cr.rec, cr.stream_id, cr.status, cr.flags, 0};
          fill += cr.fill;
          have = true;
        }
      }
      if (have && e.kind == 4) {
        if (m.status == GRDMA_H2_MSG_OK && fill + e.b <= m.length && m.offset + m.length <= A->arena_bytes) {
          pc.src = call->src_arena + call->sl[e.slice].off + e.a;
          pc.dst = A->arena + m.offset + fill;
          pc.len = e.b;
        }
      } else if (have) {  // MSG_END, or STREAM_CLOSED while the message is partial
        d.offset = m.offset;
        d.length = m.length;
        d.seq = m.seq;
        d.stream_id = m.stream;
        d.status = (e.kind == 7 && m.status == GRDMA_H2_MSG_OK) ? GRDMA_H2_MSG_TRUNCATED : m.status;
        if (d.status == GRDMA_H2_MSG_TRUNCATED) d.offset = 0;
        d.flags = m.flags;
        d.pad = 1;
        if (m.rec != ~0ull) d.pad = 1 | (uint32_t)((m.rec % A->max_pending) << 1);
        else d.pad = 1 | (0x7fffffffu << 1);
      }
    }
    // the piece's copy tiles, prefixed within the wave tile (k_h2_asm_finish adds the wave tiles in front)
    const uint64_t nct = (pc.len + H2A_COPY_TILE - 1) / H2A_COPY_TILE;
    const uint64_t cincl = wave_incl_scan(nct, lane);
    pc.tpre = cincl - nct;
    if (i < n) {
      A->pieces[i] = pc;
      A->dtmp[i] = d;
    }
    const uint64_t dm = __ballot(d.pad & 1);
    if (lane == 63) {
      A->tiles[t].nrep = (uint32_t)__builtin_popcountll(dm);
      A->tiles[t].ncopy = (uint32_t)cincl;
    }
  }
#elif H2A_STAGE == 5  // k_h2_asm_finish
  __shared__ uint64_t ws[H2A_ONE_THREADS / 64];
  __shared__ uint64_t s_nopen;
  const int tid = threadIdx.x;
  if (A->skip) return;
  const uint64_t n = A->n, ntiles = (n + 63) / 64;
  uint64_t carry = 0, ccarry = 0;
  for (uint64_t t0 = 0; t0 < ntiles; t0 += H2A_ONE_THREADS) {
    const uint64_t t = t0 + tid;
    uint64_t tot, ctot;
    const uint64_t e = h2a_block_scan(t < ntiles ? A->tiles[t].nrep : 0, ws, &tot);
    const uint64_t ce = h2a_block_scan(t < ntiles ? A->tiles[t].ncopy : 0, ws, &ctot);
    if (t < ntiles) {
      A->tiles[t].rep_base = carry + e;
      A->tiles[t].copy_base = ccarry + ce;
    }
    carry += tot;
    ccarry += ctot;
  }
  uint64_t nd = carry;
  if (tid == 0) A->ncopy = ccarry;
  __syncthreads();
  if (tid == 0) {
    // the streams' states after the call
    const uint64_t nf = A->nfin;
    for (uint64_t j = 0; j < nf; j++) {
      const h2a_key f = A->fin[j];
      const uint64_t s = h2a_tab_find(A, f.key);
      if (f.kind == H2A_SHUT) {
        if (s != ~0ull) h2a_tab_delete(A, s);
      } else if (f.kind == H2A_OPEN) {
        const h2a_msg m = A->msgs[f.idx];
        h2a_tab_put(A, h2a_carry{f.key, m.status, m.flags, 0, m.offset, m.length, m.seq, m.rec, f.bytes});
      } else if (s != ~0ull) {
        A->tab[s].fill += f.bytes;
      }
    }
    s_nopen = 0;
  }
  __syncthreads();
  // a connection error: every message still partial is truncated, reported after the others in seq order
  if (call->res->error != 0 && tid == 0) {
    uint64_t nopen = 0;
    for (uint32_t s = 0; s <= A->tab_mask; s++) {
      const h2a_carry c = A->tab[s];
      if (!c.stream_id) continue;
      // insertion by seq into the descriptors behind the event-ordered ones
      uint64_t at = nd + nopen;
      while (at > nd && A->desc[at - 1].seq > c.seq) {
        if (at < A->desc_cap) A->desc[at] = A->desc[at - 1];
        at--;
      }
      if (at < A->desc_cap)
        A->desc[at] = grdma_h2_rx_msg{0, c.length, c.seq, c.stream_id,
                                      c.status == GRDMA_H2_MSG_OK ? (uint32_t)GRDMA_H2_MSG_TRUNCATED : c.status, c.flags, 0};
      if (c.rec != ~0ull) A->recs[c.rec % A->max_pending].freed = 1;
      if (c.status == GRDMA_H2_MSG_OK || c.status == GRDMA_H2_MSG_TRUNCATED) A->st_trunc++;
      else if (c.status == GRDMA_H2_MSG_TOO_LARGE) A->st_too_large++;
      else A->st_no_space++;
      nopen++;
    }
    for (uint32_t s = 0; s <= A->tab_mask; s++) A->tab[s].stream_id = 0;
    s_nopen = nopen;
  }
  __syncthreads();
  if (tid == 0) {
    const uint64_t tot = nd + s_nopen;
    // ranks of the truncated-at-error descriptors (the event-ordered ones get theirs in k_h2_asm_copy)
    for (uint64_t j = nd; j < tot && j < A->desc_cap; j++) A->desc[j].pad = 0;
    A->rank_base = A->reported;
    A->reported += tot;
    A->st_reported += tot;
    A->ndesc = tot;
    // records: head after the call
    uint64_t ns = A->cutoff;
    A->rec_head = A->rec_base + ns;
    // virtual head: behind the last message allocated
    if (ns) {
      const h2a_rec& last = A->recs[(A->rec_base + ns - 1) % A->max_pending];
      if (last.vend > A->vh) A->vh = last.vend;
    }
  }
#elif H2A_STAGE == 6  // k_h2_asm_copy, descriptors: wave `wave` of `waves` places those of the wave tiles it owns (n, ntiles, lane
                      // and the four counters ok_bytes, too_large, no_space, trunc in scope)
  for (uint64_t t = wave; t < ntiles; t += waves) {
    const uint64_t i = t * 64 + lane;
    grdma_h2_rx_msg d{0, 0, 0, 0, 0, 0, 0};
    if (i < n) d = A->dtmp[i];
    const bool rep = d.pad & 1;
    const uint64_t dm = __ballot(rep);
    if (rep) {
      const uint64_t pos = A->tiles[t].rep_base + (uint64_t)__builtin_popcountll(dm & ((1ull << lane) - 1));
      const uint32_t recslot = d.pad >> 1;
      d.pad = 0;
      if (pos < A->desc_cap) A->desc[pos] = d;
      if (recslot != 0x7fffffffu) {
        h2a_rec& rc = A->recs[recslot];
        rc.rank = A->rank_base + pos;
        if (d.status == GRDMA_H2_MSG_TRUNCATED) rc.freed = 1;
      }
      if (d.status == GRDMA_H2_MSG_OK) ok_bytes += d.length;
      else if (d.status == GRDMA_H2_MSG_TOO_LARGE) too_large++;
      else if (d.status == GRDMA_H2_MSG_NO_SPACE) no_space++;
      else trunc++;
    }
  }
#elif H2A_STAGE == 7  // k_h2_asm_copy, lookup: copy tile c of the call -> src, dst, len (n, ntiles in scope)
      const uint64_t t = h2a_last_le_tile(A, ntiles, c);
      const uint64_t local = c - A->tiles[t].copy_base;
      // the last piece of wave tile t whose tpre <= local (a piece without tiles shares its tpre with the next)
      uint64_t lo = 0, hi = 64;
      if (t * 64 + hi > n) hi = n - t * 64;
      while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (A->pieces[t * 64 + mid].tpre <= local) lo = mid;
        else hi = mid;
      }
      const h2a_piece pc = A->pieces[t * 64 + lo];
      const uint64_t off = (local - pc.tpre) * H2A_COPY_TILE;
      if (off < pc.len) {
        src = pc.src + off;
        dst = pc.dst + off;
        len = pc.len - off < H2A_COPY_TILE ? pc.len - off : H2A_COPY_TILE;
      }
#endif
