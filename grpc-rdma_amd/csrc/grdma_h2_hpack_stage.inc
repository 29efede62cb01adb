// The bodies of the header decoder's stages as source text, included by the single-transport kernels (k_h2_hpack_*:
// H2HP_BLK = blockIdx.x, H2HP_NBLK = H2HP_GRID), csrc/grdma_h2_hpack.h; a family over a table of links can include the
// same text with a link's share of the grid.  H2HP_STAGE selects the stage; every stage expects `h2hp_dev* F` and
// `const h2hp_call* call` in scope, as the kernels' parameters are.  (Source text rather than device functions, as
// csrc/grdma_h2_ctl_stage.inc.)
#if H2HP_STAGE == 1  // k_h2_hpack_gather: one workgroup
  __shared__ uint64_t s_wave[H2HP_THREADS / 64];
  __shared__ uint32_t s_last, s_closes;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    s_last = s_closes = 0;
    F->carry_out = h2hp_carry{0, 0, 0, 0, H2HP_NONE, 0, 0, 0, 0, {0, 0, 0}};
    for (int k = 0; k < 4; k++) F->pre[k] = 0;
  }
  __syncthreads();
  // (uniform) a call that is taken without being read: the walk says why
  if ((F->sticky & (H2HP_F_FAILED | H2HP_F_LOST)) || h2hp_lost(call) || call->skipped || call->res->error != 0) return;
  const uint64_t n = call->res->nevents, nit = n + 1;  // item 0: the carried frame and block; item t: event t - 1
  const h2hp_carry cy = F->carry;
  const uint64_t low40 = (1ull << 40) - 1;
  uint64_t base = 0;  // fragment bytes | blocks << 40 in front of the step
  for (uint64_t c0 = 0; c0 < nit; c0 += H2HP_THREADS) {  // (uniform: the scan's barriers)
    const uint64_t t = c0 + tid;
    bool hdr = false, start = false;
    uint32_t frag = 0, err = 0, stream = 0, bflags = 0, closes = 0;
    h2hp_item it = {0, 0, 0, 0};
    if (t < nit) {
      uint32_t type1 = 0, flags = 0, size = 0, seen0 = 0, pad = H2HP_NONE;
      if (t == 0) {
        type1 = cy.type1;
        flags = cy.flags;
        size = cy.size;
        seen0 = cy.seen;
        pad = cy.pad;
        if (cy.in_block) {
          hdr = start = true;
          frag = cy.frag_len;
          stream = cy.blk_stream;
          bflags = cy.blk_flags;
        }
      } else {
        const grdma_h2_event e = call->ev[t - 1];
        if (e.kind == EV_FRAME && e.a != 0xffu) {
          type1 = e.a + 1u;
          flags = e.b & 0xffu;
          size = e.d;
          if (e.a == FT_HEADERS) {
            hdr = start = true;
            stream = e.c;
            bflags = (flags & 1u) | ((flags & 0x20u) ? 2u : 0u) | (((e.b >> 8) & 0xffu) << 8);
          } else if (e.a == FT_CONTINUATION) {
            hdr = true;
          }
        }
      }
      if (type1) {
        const uint32_t type = type1 - 1u;
        const bool padded = type == FT_HEADERS && (flags & 0x8u);
        uint32_t pos = seen0;
        const bool complete = h2hp_walk_frame(call, t, n, padded, pos, pad);
        if (!complete) {  // (at most one frame of a call: the last one)
          F->carry_out.type1 = type1;
          F->carry_out.flags = flags;
          F->carry_out.size = size;
          F->carry_out.seen = pos;
          F->carry_out.pad = pad;
        }
        if (hdr && h2hp_is_header(type)) {
          const uint32_t lo = h2hp_lo(type, flags);
          uint32_t hi = 0;
          if (size < lo) err = H2HP_E_PADDING;
          else if (!padded) hi = size;
          else if (pad != H2HP_NONE) {
            if (pad >= size - lo) err = H2HP_E_PADDING;
            else hi = size - pad;
          }
          const uint32_t a = lo > seen0 ? lo : seen0, b = hi < pos ? hi : pos;
          if (!err && b > a) {
            frag += b - a;
            it = h2hp_item{0, a, b, seen0};
          }
          closes = (complete && (flags & 0x4u)) ? 1u : 0u;
        }
      }
    }
    uint64_t tot;
    const uint64_t x = base + block_excl_scan((uint64_t)frag | ((uint64_t)(start ? 1 : 0) << 40), s_wave, &tot);
    if (hdr) {
      const uint32_t off = (uint32_t)(x & low40);
      it.dst = off + (t == 0 ? cy.frag_len : 0u);  // (the carried fragment stands in front of item 0's new bytes)
      if (start && (x >> 40) < F->items_cap) F->blks[x >> 40] = h2hp_blk{off, 0, stream, bflags, err, 0, 0, 0};
      atomicMax(&s_last, (uint32_t)t + 1u);
    }
    if (t < nit && t < F->items_cap) F->items[t] = it;
    base += tot;
    __syncthreads();
    if (hdr && (uint32_t)t + 1u == s_last) s_closes = closes;  // (the last header frame so far)
  }
  __syncthreads();
  if (tid == 0) {
    F->pre[0] = base & low40;
    F->pre[1] = base >> 40;
    F->pre[2] = ((base >> 40) && !s_closes) ? 1 : 0;
  }
#elif H2HP_STAGE == 2  // k_h2_hpack_copy
  const uint64_t total = F->pre[0] < F->stage_cap ? F->pre[0] : F->stage_cap;
  if (total == 0) return;  // (uniform)
  const uint64_t n = call->res->nevents, nit = n + 1 < F->items_cap ? n + 1 : F->items_cap;
  const uint64_t gtid = (uint64_t)H2HP_BLK * H2HP_THREADS + threadIdx.x, gsz = (uint64_t)H2HP_NBLK * H2HP_THREADS;
  uint8_t* const stage = F->stage;
  const uint64_t carried = F->carry.in_block ? F->carry.frag_len : 0;
  for (uint64_t i = gtid; i < carried && i < total; i += gsz) stage[i] = F->carry_buf[i];
  for (uint64_t t = gtid; t < nit; t += gsz) {
    const h2hp_item it = F->items[t];
    if (it.lo >= it.hi) continue;
    uint32_t pos = it.seen0;
    uint64_t dst = it.dst;
    for (uint64_t j = t; j < n; j++) {  // the frame's PAYLOAD events: bounded as h2hp_walk_frame
      const grdma_h2_event e = call->ev[j];
      if (e.kind == EV_FRAME) {
        if (e.a != 0xffu) break;
        continue;
      }
      if (e.kind != EV_PAYLOAD) continue;
      const uint32_t a = it.lo > pos ? it.lo : pos, b = it.hi < pos + e.b ? it.hi : pos + e.b;
      if (b > a) {
        const uint8_t* src = h2hp_piece(call, e);
        for (uint32_t k = a; k < b; k++, dst++)
          if (dst < total) stage[dst] = src ? src[k - pos] : (uint8_t)0;
      }
      pos += e.b;
      if (e.c || pos >= it.hi) break;
    }
  }
#elif H2HP_STAGE == 3  // k_h2_hpack_split
  __shared__ uint32_t s_A[H2HP_HUFF_WORDS];
  const uint64_t nblk = F->pre[1] < F->items_cap ? F->pre[1] : F->items_cap;
  if (nblk == 0) return;  // (uniform)
  for (uint32_t i = threadIdx.x; i < H2HP_HUFF_WORDS; i += H2HP_THREADS) s_A[i] = F->huff[i];
  __syncthreads();
  const uint64_t total = F->pre[0] < F->stage_cap ? F->pre[0] : F->stage_cap;
  const uint64_t ndone = nblk - (F->pre[2] ? 1 : 0);
  const uint64_t gtid = (uint64_t)H2HP_BLK * H2HP_THREADS + threadIdx.x, gsz = (uint64_t)H2HP_NBLK * H2HP_THREADS;
  for (uint64_t k = gtid; k < nblk; k += gsz) {
    const h2hp_blk B = F->blks[k];
    const uint32_t end_off = k + 1 < nblk ? F->blks[k + 1].off : (uint32_t)total;
    const uint32_t len = end_off > B.off && B.off <= total ? end_off - B.off : 0u;
    uint32_t err = B.err, nrec = 0, nfields = 0;
    if (!err && len > F->max_block) err = H2HP_E_BLOCK_TOO_LARGE;
    if (!err && k < ndone) {  // a complete block: its fields.  Every step takes at least one of the block's len bytes.
      const uint8_t* blk = F->stage + B.off;
      uint32_t pos = 0;
      while (pos < len && !err) {
        h2hp_rec r = {0, 0, 0, 0, 0, 0, 0, (uint32_t)k};
        const uint32_t b = blk[pos];
        uint32_t v = 0;
        if (b & 0x80u) {
          err = h2hp_int(blk, pos, len, 7, v);
          r.w0 = v < 0xffffffu ? v : 0xffffffu;  // (an index that large is none)
        } else if ((b & 0xe0u) == 0x20u) {
          err = h2hp_int(blk, pos, len, 5, v);
          if (!err && (nfields || v > F->setting)) err = H2HP_E_SIZE_UPDATE;
          r.w0 = v | (1u << 28);
        } else {
          const uint32_t rep = (b & 0x40u) ? 1u : (b & 0x10u) ? 3u : 2u;
          err = h2hp_int(blk, pos, len, rep == 1u ? 6 : 4, v);
          r.w0 = (v < 0xffffffu ? v : 0xffffffu) | (rep << 24);
          if (!err && v == 0) {
            r.name_pos = B.off + pos;
            err = h2hp_string(s_A, blk, pos, len, r.name_len);
          }
          if (!err) {
            r.value_pos = B.off + pos;
            err = h2hp_string(s_A, blk, pos, len, r.value_len);
          }
        }
        if (err) break;
        if ((uint64_t)B.off + nrec < F->recs_cap) F->recs[B.off + nrec] = r;
        nrec++;
        nfields += (r.w0 >> 28) ? 0u : 1u;
      }
    }
    F->blks[k].len = len;
    F->blks[k].err = err;
    F->blks[k].nrec = nrec;
    F->blks[k].nfields = nfields;
  }
#elif H2HP_STAGE == 4  // k_h2_hpack_walk: one workgroup
  __shared__ h2hp_entry s_ring[H2HP_RING];
  __shared__ uint32_t s_out[H2HP_RING];  // where the strings of an entry this call inserted stand in the string arena
  __shared__ h2hp_rec s_rec[H2HP_CHUNK];
  __shared__ uint64_t s_wave[H2HP_THREADS / 64];
  __shared__ uint16_t s_stlen[128];
  __shared__ uint32_t s_bad, s_m, s_count, s_q, s_cnt, s_ins, s_add, s_isfield, s_fail, s_fail1, s_commit;
  const uint32_t tid = threadIdx.x;
  const uint32_t mask = H2HP_RING - 1u;
  const uint64_t sticky = F->sticky;
  {
    const bool dead = (sticky & (H2HP_F_FAILED | H2HP_F_LOST)) != 0, lost = h2hp_lost(call);
    if (dead || lost || call->skipped || call->res->error != 0) {  // (uniform) taken, nothing written, the carry goes
      if (tid == 0) {
        const uint64_t w = dead ? sticky : sticky | ((lost || call->skipped) ? (uint64_t)H2HP_F_LOST : (uint64_t)(H2HP_F_FAILED | (H2HP_E_DEFRAMER << 8)));
        F->sticky = w;
        F->carry = h2hp_carry{0, 0, 0, 0, H2HP_NONE, 0, 0, 0, 0, {0, 0, 0}};
        F->st_calls++;
        for (int k = 0; k < 8; k++) F->res[k] = 0;
        F->res[H2HP_TABLE] = F->size;
        F->res[H2HP_FLAGS] = w;
        F->res[H2HP_OVERFLOW] = (!dead && lost) ? 2 : 0;
        F->good_blocks = F->njobs = F->open_len = 0;
      }
      return;
    }
  }
  const uint32_t nblk = (uint32_t)(F->pre[1] < F->items_cap ? F->pre[1] : F->items_cap), open = F->pre[2] ? 1u : 0u;
  const uint32_t ndone = nblk - open;
  if (tid == 0) s_bad = nblk;
  if (tid < 124) s_stlen[tid] = (uint16_t)(F->st_off[tid + 1] - F->st_off[tid]);
  __syncthreads();
  for (uint32_t k = tid; k < nblk; k += H2HP_THREADS)
    if (F->blks[k].err) atomicMin(&s_bad, k);
  __syncthreads();
  uint32_t bad = s_bad, bad_err = 0;               // the first failing block (nblk: none); H2HP_E_INDEX where the walk finds it
  uint32_t limit = bad < ndone ? bad : ndone;      // blocks [0, limit) are delivered
  // thread 0's: the table; every thread's (uniform): the call's fields and string bytes so far
  uint32_t cur_max = 0, size = 0, cnt = 0, ins = 0, inserted = 0, evicted = 0;
  uint64_t nfields = 0, run = 0;
  for (int pass = 0; pass < 2; pass++) {  // (uniform) an index error in block k: once more over the blocks in front of it
    for (uint32_t i = tid; i < H2HP_RING; i += H2HP_THREADS) s_ring[i] = F->ring[i];
    if (tid == 0) {
      cur_max = F->cur_max;
      size = F->size;
      cnt = F->cnt;
      ins = F->ins;
      inserted = evicted = 0;
      s_cnt = cnt;
      s_ins = ins;
      s_fail = s_fail1 = H2HP_NONE;
    }
    nfields = run = 0;
    __syncthreads();
    uint32_t k0 = 0, f0 = 0;      // (uniform) the next block, and the next record of it where it is taken in pieces
    uint64_t first = 0;           // fields in front of block k0
    while (k0 < limit) {
      // how many blocks from k0 on fit the staged records: thread t looks at block k0 + t
      const uint32_t kb = k0 + tid;
      const h2hp_blk B = kb < limit ? F->blks[kb] : h2hp_blk{0, 0, 0, 0, 0, 0, 0, 0};
      uint64_t tot;
      const uint64_t x = block_excl_scan((uint64_t)B.nrec | ((uint64_t)B.nfields << 32), s_wave, &tot);
      const uint32_t xr = (uint32_t)x;
      if (tid == 0) s_m = s_count = 0;
      __syncthreads();
      if (f0 == 0 && kb < limit && (uint64_t)xr + B.nrec <= H2HP_CHUNK) atomicMax(&s_m, tid + 1u);  // (a prefix: the count)
      __syncthreads();
      const uint32_t m = s_m;
      if (m) {
        if (tid < m) {
          for (uint32_t j = 0; j < B.nrec; j++)
            if ((uint64_t)B.off + j < F->recs_cap) s_rec[xr + j] = F->recs[B.off + j];
          F->blks[kb].first = (uint32_t)(first + (x >> 32));
          if (tid == m - 1u) s_count = xr + B.nrec;
        }
      } else {  // block k0 has more records than fit: H2HP_CHUNK of them from f0 on (B of thread 0 is block k0)
        const h2hp_blk B0 = F->blks[k0];
        const uint32_t c = B0.nrec - f0 < H2HP_CHUNK ? B0.nrec - f0 : H2HP_CHUNK;
        for (uint32_t j = tid; j < c; j += H2HP_THREADS)
          if ((uint64_t)B0.off + f0 + j < F->recs_cap) s_rec[j] = F->recs[B0.off + f0 + j];
        if (tid == 0) {
          s_count = c;
          if (f0 == 0) F->blks[k0].first = (uint32_t)first;
        }
      }
      __syncthreads();
      const uint32_t count = s_count;
      const uint64_t out0 = nfields;
      uint32_t p = 0, o = 0;  // (uniform) the next record; the fields of this step so far
      while (p < count) {
        // The records from p up to the next one that changes the table -- an insertion, a size update -- see ONE table:
        // every thread takes one, a block scan over their lengths gives the offsets in the string arena.
        if (tid == 0) s_q = count;
        __syncthreads();
        for (uint32_t i = p + tid; i < count; i += H2HP_THREADS) {
          const uint32_t w0 = s_rec[i].w0;
          if ((w0 >> 28) || ((w0 >> 24) & 3u) == 1u) {
            atomicMin(&s_q, i);
            break;
          }
        }
        __syncthreads();
        const uint32_t q = s_q, t_cnt = s_cnt, t_ins = s_ins;
        for (uint32_t i0 = p; i0 < q; i0 += H2HP_THREADS) {  // (uniform: the scan's barriers)
          const uint32_t i = i0 + tid;
          h2hp_rec r = {0, 0, 0, 0, 0, 0, 0, 0};
          uint32_t nsrc = 0, nlen = 0, vsrc = 0, vlen = 0;
          bool ok = false;
          if (i < q) {
            r = s_rec[i];
            ok = h2hp_resolve(r, s_ring, s_stlen, t_cnt, t_ins, nsrc, nlen, vsrc, vlen);
            if (!ok) atomicMin(&s_fail, r.rsv);
          }
          uint64_t tot;
          const uint64_t x = run + block_excl_scan(ok ? (uint64_t)nlen + vlen : 0ull, s_wave, &tot);
          // (in place: field o + (i - p) stands at or in front of record i, and this step's records are read)
          if (ok) s_rec[o + (i - p)] = h2hp_rec{(r.w0 >> 24) & 3u, nsrc, vsrc, nlen, vlen, (uint32_t)x, (uint32_t)(x + nlen), r.rsv};
          run += tot;
        }
        o += q - p;
        __syncthreads();
        if (s_fail != H2HP_NONE) break;  // (uniform)
        if (q < count) {  // the record that changes the table: one thread
          if (tid == 0) {
            const h2hp_rec r = s_rec[q];
            s_add = s_isfield = 0;
            if (r.w0 >> 28) {
              cur_max = r.w0 & 0xffffffu;
              H2HP_EVICT(s_ring, 0u, cur_max);
            } else {
              uint32_t nsrc = 0, nlen = 0, vsrc = 0, vlen = 0;
              if (!h2hp_resolve(r, s_ring, s_stlen, cnt, ins, nsrc, nlen, vsrc, vlen)) {
                s_fail1 = r.rsv;  // (a word of its own: a thread may still be reading s_fail in front of this step)
              } else {  // (the name was resolved before this evicts: RFC 7541 4.4)
                const uint64_t need = 32ull + nlen + vlen;
                H2HP_EVICT(s_ring, need, cur_max);
                if (need <= cur_max) {
                  s_ring[ins & mask] = h2hp_entry{nsrc, nlen, vsrc, vlen};
                  s_out[ins & mask] = (uint32_t)run;
                  ins++;
                  cnt++;
                  size += (uint32_t)need;
                  inserted++;
                }
                s_rec[o] = h2hp_rec{1u, nsrc, vsrc, nlen, vlen, (uint32_t)run, (uint32_t)(run + nlen), r.rsv};
                s_add = nlen + vlen;
                s_isfield = 1;
              }
            }
            s_cnt = cnt;
            s_ins = ins;
          }
          __syncthreads();
          if (s_fail1 != H2HP_NONE) break;  // (uniform)
          o += s_isfield;
          run += s_add;
        }
        p = q + 1u;
      }
      nfields += o;
      __syncthreads();
      if (s_fail != H2HP_NONE || s_fail1 != H2HP_NONE) break;  // (uniform)
      // the resolved fields go out, behind those of the steps in front (thread 0 holds the count: through LDS)
      if (tid == 0) s_wave[0] = out0;
      if (m && tid == m - 1u) s_wave[1] = (x >> 32) + B.nfields;  // the fields of the m blocks
      __syncthreads();
      const uint64_t o0 = s_wave[0];
      for (uint32_t i = tid; i < o; i += H2HP_THREADS)
        if (o0 + i < F->outs_cap) F->outs[o0 + i] = s_rec[i];
      if (m) {
        first += s_wave[1];
        k0 += m;
      } else {
        f0 += count;
        const h2hp_blk B0 = F->blks[k0];
        if (f0 >= B0.nrec) {  // (uniform) the block is through
          first += B0.nfields;
          k0++;
          f0 = 0;
        }
      }
      __syncthreads();
    }
    const uint32_t fail = s_fail < s_fail1 ? s_fail : s_fail1;  // (the runs' threads, or thread 0 at an insertion)
    if (fail == H2HP_NONE) break;
    bad = fail;  // (in front of every block that failed the split: those were not walked)
    bad_err = H2HP_E_INDEX;
    limit = bad;
    __syncthreads();
  }
  if (tid == 0) {
    const bool failed = bad < nblk;
    uint64_t word = sticky;
    if (failed) word |= H2HP_F_FAILED | ((uint64_t)(bad_err ? bad_err : F->blks[bad].err) << 8) | ((uint64_t)F->blks[bad].stream << 32);
    const bool over = limit > F->blocks_cap || nfields > F->fields_cap || run > F->strings_cap;
    F->res[H2HP_BLOCKS] = limit;
    F->res[H2HP_FIELDS] = nfields;
    F->res[H2HP_STRINGS] = run;
    F->res[H2HP_INSERTED] = inserted;
    F->res[H2HP_EVICTED] = evicted;
    F->res[H2HP_TABLE] = size;
    F->res[H2HP_FLAGS] = word | ((open && !failed) ? (uint64_t)H2HP_F_OPEN : 0ull);
    F->res[H2HP_OVERFLOW] = over ? 1 : 0;
    F->good_blocks = over ? 0u : limit;
    F->njobs = F->open_len = 0;
    s_commit = over ? 0u : 1u;
    if (!over) {
      // the entries this call inserted and that live get their place in the byte ring, behind the older ones
      const uint32_t fresh = ins - F->ins < cnt ? ins - F->ins : cnt;
      uint32_t head = F->ring_head, nj = 0;
      for (uint32_t q = 0; q < fresh; q++) {
        const uint32_t slot = (ins - fresh + q) & mask;
        h2hp_entry e = s_ring[slot];
        F->jobs[nj++] = h2hp_job{s_out[slot], head, e.name_len + e.value_len, 0};
        e.name_src = H2HP_SRC(H2HP_S_RING, head);
        e.value_src = H2HP_SRC(H2HP_S_RING, (head + e.name_len) & (H2HP_BYTES - 1u));
        head = (head + e.name_len + e.value_len) & (H2HP_BYTES - 1u);
        s_ring[slot] = e;
      }
      F->njobs = nj;
      F->ring_head = head;
      F->cur_max = cur_max;
      F->size = size;
      F->cnt = cnt;
      F->ins = ins;
      F->sticky = word;
      F->st_calls++;
      F->st_blocks += limit;
      F->st_fields += nfields;
      F->st_strings += run;
      F->st_inserted += inserted;
      F->st_evicted += evicted;
      h2hp_carry c = F->carry_out;
      if (failed) {
        c = h2hp_carry{0, 0, 0, 0, H2HP_NONE, 0, 0, 0, 0, {0, 0, 0}};
      } else if (open) {
        const h2hp_blk B = F->blks[nblk - 1u];
        c.in_block = 1;
        c.blk_stream = B.stream;
        c.blk_flags = B.flags;
        c.frag_len = B.len;
        F->open_off = B.off;
        F->open_len = B.len;
      }
      F->carry = c;
    }
  }
  __syncthreads();
  if (s_commit)
    for (uint32_t i = tid; i < H2HP_RING; i += H2HP_THREADS) F->ring[i] = s_ring[i];
#elif H2HP_STAGE == 5  // k_h2_hpack_emit
  __shared__ uint32_t s_A[H2HP_HUFF_WORDS];
  const uint64_t nb = F->res[H2HP_BLOCKS], nf = F->res[H2HP_FIELDS], ns = F->res[H2HP_STRINGS];
  if (F->res[H2HP_OVERFLOW] || nb == 0) return;  // (uniform) nothing half-written
  for (uint32_t i = threadIdx.x; i < H2HP_HUFF_WORDS; i += H2HP_THREADS) s_A[i] = F->huff[i];
  __syncthreads();
  const uint64_t gtid = (uint64_t)H2HP_BLK * H2HP_THREADS + threadIdx.x, gsz = (uint64_t)H2HP_NBLK * H2HP_THREADS;
  const uint32_t total = (uint32_t)(F->pre[0] < F->stage_cap ? F->pre[0] : F->stage_cap);
  for (uint64_t q = gtid; q < 2 * nf; q += gsz) {  // one string a lane
    if ((q >> 1) >= F->outs_cap) break;
    const h2hp_rec r = F->outs[q >> 1];
    const uint32_t src = (q & 1) ? r.value_pos : r.name_pos, len = (q & 1) ? r.value_len : r.name_len;
    const uint64_t off = (q & 1) ? r.value_off : r.name_off;
    if (off + len > ns) continue;  // (cannot fail: the walk summed the same lengths)
    uint8_t* dst = F->strings + off;
    const uint32_t kind = src >> 30, p = src & 0x3fffffffu;
    if (kind == H2HP_S_STATIC) {
      const uint8_t* b = F->st_bytes + F->st_off[2u * (p & 255u) + (p >> 8)];
      for (uint32_t k = 0; k < len; k++) dst[k] = b[k];
    } else if (kind == H2HP_S_RING) {
      for (uint32_t k = 0; k < len; k++) dst[k] = F->bytes[(p + k) & (H2HP_BYTES - 1u)];
    } else {
      const uint8_t* blk = F->stage;
      uint32_t pos = p, n = 0;
      if (pos >= total) continue;
      const uint32_t h = blk[pos] & 0x80u;
      if (h2hp_int(blk, pos, total, 7, n) || n > total - pos) continue;  // (cannot fail: the split read the same bytes)
      if (h) h2hp_huffman(s_A, blk + pos, n, dst, len);
      else for (uint32_t k = 0; k < len && k < n; k++) dst[k] = blk[pos + k];
    }
  }
  for (uint64_t i = gtid; i < nf && i < F->outs_cap; i += gsz) {
    const h2hp_rec r = F->outs[i];
    F->fields[i] = h2hp_field_out{r.name_off, r.value_off, r.name_len | (r.w0 << 24), r.value_len};
  }
  for (uint64_t k = gtid; k < nb && k < F->items_cap; k += gsz) {
    const h2hp_blk B = F->blks[k];
    F->blocks[k] = h2hp_block_out{B.stream, B.first, B.nfields, B.flags};
  }
#elif H2HP_STAGE == 6  // k_h2_hpack_commit
  if (F->res[H2HP_OVERFLOW]) return;  // (uniform) nothing is committed
  const uint64_t gtid = (uint64_t)H2HP_BLK * H2HP_THREADS + threadIdx.x, gsz = (uint64_t)H2HP_NBLK * H2HP_THREADS;
  const uint64_t ns = F->res[H2HP_STRINGS];
  const uint32_t nj = F->njobs < H2HP_RING ? F->njobs : H2HP_RING;
  for (uint64_t j = gtid; j < nj; j += gsz) {
    const h2hp_job job = F->jobs[j];
    for (uint32_t k = 0; k < job.len; k++)
      if ((uint64_t)job.src + k < ns) F->bytes[(job.dst + k) & (H2HP_BYTES - 1u)] = F->strings[job.src + k];
  }
  const uint64_t keep = F->open_len < F->max_block ? F->open_len : F->max_block;
  for (uint64_t i = gtid; i < keep; i += gsz)
    if ((uint64_t)F->open_off + i < F->stage_cap) F->carry_buf[i] = F->stage[F->open_off + i];
#elif H2HP_STAGE == 7  // k_h2_hpack_resize: our setting changed (the host wrote it); a lowered one takes effect at once
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t cur_max = F->cur_max, size = F->size, cnt = F->cnt, evicted = 0;
  const uint32_t ins = F->ins;
  if (cur_max > F->setting) {
    cur_max = F->setting;
    H2HP_EVICT(F->ring, 0u, cur_max);
    F->cur_max = cur_max;
    F->size = size;
    F->cnt = cnt;
    F->st_evicted += evicted;
  }
#else
#error "H2HP_STAGE: 1 gather, 2 copy, 3 split, 4 walk, 5 emit, 6 commit, 7 resize"
#endif
