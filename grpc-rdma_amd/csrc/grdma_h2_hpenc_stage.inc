// The bodies of the header encoder's stages as source text, included by the single-connection kernels (k_h2_hpenc_*:
// H2HE_BLK = blockIdx.x, H2HE_NBLK = H2HE_GRID) and by the kernels over a table of links (k_h2_links_hpenc_*: a link's
// share of the grid), csrc/grdma_h2_hpenc.h.  H2HE_STAGE selects the stage.  Every stage expects in scope, as the
// including kernel names them:
//   h2he_dev* F          the encoder block: state, counters, the hand-overs between the launches (go, njobs, jobs, nocc's
//                        reader aside) and the tables
//   const h2he_call* C   the call's words (&F->c in the single kernels, the item's words of the batch block over links)
//   uint64_t* R          the eight result words the host reads (F->res, or the item's words of the batch block)
//   uint64_t* N          the occurrence count behind them (&F->nocc, or R + 8)
// (Source text rather than device functions, as csrc/grdma_h2_hpack_stage.inc.)
#if H2HE_STAGE == 1  // k_h2_hpenc_scan: a lane per field of the field table
  __shared__ uint8_t s_bits[256];
  __shared__ uint32_t s_hn[64], s_hf[64];
  __shared__ uint16_t s_off[2 * 62 + 2];
  const uint32_t tid = threadIdx.x;
  s_bits[tid] = F->huff_bits[tid];
  if (tid < 64) {
    s_hn[tid] = F->st_hn[tid];
    s_hf[tid] = F->st_hf[tid];
  }
  if (tid < 2 * 62 + 2) s_off[tid] = F->st_off[tid];
  __syncthreads();
  const uint64_t nf = C->nfields < C->recs_cap ? C->nfields : C->recs_cap, ns = C->strings_bytes;
  const uint64_t gtid = (uint64_t)(H2HE_BLK) * H2HE_THREADS + tid, gsz = (uint64_t)(H2HE_NBLK) * H2HE_THREADS;
  for (uint64_t i = gtid; i < nf; i += gsz) {
    const h2hp_field_out f = C->fields[i];
    const uint32_t nl = f.name_len & 0xffffffu, vl = f.value_len;
    h2he_rec r = {0, 0, 0, 0, 0, {0, 0, 0}};
    if (vl > 0xffffffu) r.st = (uint32_t)H2HE_E_LENGTH << 16;
    else if ((uint64_t)f.name_off + nl > ns || (uint64_t)f.value_off + vl > ns) r.st = (uint32_t)H2HE_E_STRING << 16;
    if (r.st) {
      C->recs[i] = r;
      continue;
    }
    const uint8_t* name = C->strings + f.name_off;
    const uint8_t* value = C->strings + f.value_off;
    uint32_t h = 0x811c9dc5u;
    uint64_t nb = 0;
    for (uint32_t k = 0; k < nl; k++) {
      const uint32_t b = name[k];
      h = h2he_fnv(h, b);
      nb += s_bits[b];
    }
    r.hn = h;
    nb = (nb + 7u) >> 3;
    r.nenc = (nl && nb <= nl) ? (uint32_t)nb | 0x80000000u : nl;  // (Huffman where that is not longer: RFC 7541 C.6.2)
    nb = 0;
    for (uint32_t k = 0; k < vl; k++) {
      const uint32_t b = value[k];
      h = h2he_fnv(h, b);
      nb += s_bits[b];
    }
    r.hf = h;
    nb = (nb + 7u) >> 3;
    r.venc = (vl && nb <= vl) ? (uint32_t)nb | 0x80000000u : vl;
    uint32_t sname = 0, sfull = 0;
    for (uint32_t q = 1; q < 62u && !sfull; q++) {  // (hashes nominate, bytes decide)
      if (s_hn[q] != r.hn || (uint32_t)(s_off[2u * q + 1u] - s_off[2u * q]) != nl || !h2he_eq(F->st_bytes, s_off[2u * q], 0xffffffffu, name, nl)) continue;
      if (!sname) sname = q;
      if (s_hf[q] == r.hf && (uint32_t)(s_off[2u * q + 2u] - s_off[2u * q + 1u]) == vl && h2he_eq(F->st_bytes, s_off[2u * q + 1u], 0xffffffffu, value, vl)) sfull = q;
    }
    r.st = sfull | (sname << 8);
    C->recs[i] = r;
  }

#elif H2HE_STAGE == 2  // k_h2_hpenc_walk: one workgroup
  __shared__ uint32_t s_hn[H2HP_RING], s_hf[H2HP_RING], s_nl[H2HP_RING], s_vl[H2HP_RING], s_ns[H2HP_RING], s_vs[H2HP_RING];
  __shared__ uint64_t s_wave[H2HE_THREADS / 64];
  __shared__ uint64_t s_occ0[H2HE_CHUNK + 1];  // the occurrences in front of the blocks [kb, kb + 257): a step's blocks, mostly
  // the table (the one thread's between barriers), the round's inserting thread and what it inserted, the first bad block,
  // the first bad occurrence, the first block whose frames pass 2^32 - 1 bytes
  __shared__ uint32_t s_cur_max, s_size, s_cnt, s_ins, s_inserted, s_evicted, s_p, s_new, s_badblk, s_badocc, s_big, s_commit, s_kb;
  const uint32_t tid = threadIdx.x, mask = H2HP_RING - 1u;
  const uint32_t nblk = (uint32_t)C->nblocks;
  const uint32_t ins0 = F->ins;  // entries from here on are this call's: their strings stand in the string arena
  if (tid == 0) {
    s_badblk = s_badocc = s_big = H2HE_NONE;
    s_commit = 0;
    F->go = F->njobs = 0;
  }
  __syncthreads();
  // ---- the blocks: ranges and stream ids; the occurrences in front of each
  uint64_t nocc = 0;
  for (uint32_t k0 = 0; k0 < nblk; k0 += H2HE_THREADS) {  // (uniform: the scan's barriers)
    const uint32_t k = k0 + tid;
    uint32_t n = 0;
    if (k < nblk) {
      const h2hp_block_out B = C->blocks[k];
      if ((uint64_t)B.first_field + B.nfields > C->nfields || B.stream == 0 || B.stream > 0x7fffffffu) atomicMin(&s_badblk, k);
      else n = B.nfields;
    }
    uint64_t tot;
    const uint64_t x = nocc + block_excl_scan((uint64_t)n, s_wave, &tot);
    if (k < nblk) C->blks[k].occ0 = x;
    nocc += tot;
  }
  if (tid == 0) C->blks[nblk].occ0 = nocc;
  __syncthreads();
  const uint32_t lim = s_badblk < nblk ? s_badblk : nblk;  // blocks [0, lim) are walked (a bad string in front of a bad block is first)
  const uint64_t nwalk = C->blks[lim].occ0;
  if (nwalk > C->occs_cap) {  // (uniform) the host's table is too small: nothing is written or committed, it grows and repeats
    if (tid == 0) {
      for (int k = 0; k < 8; k++) R[k] = 0;
      R[H2HE_OVERFLOW] = H2HE_OVER_SCRATCH;
      *N = nwalk;
    }
    return;
  }
  for (uint32_t i = tid; i < H2HP_RING; i += H2HE_THREADS) {
    s_hn[i] = F->r_hn[i];
    s_hf[i] = F->r_hf[i];
    const uint32_t nl = F->r_nl[i], src = F->r_src[i];
    s_nl[i] = nl;
    s_vl[i] = F->r_vl[i];
    s_ns[i] = src;
    s_vs[i] = (src + nl) & (H2HP_BYTES - 1u);
  }
  uint32_t lead = 0;  // (uniform) the bytes of the size updates in front of block 0
  if (nblk)
    for (uint32_t u = 0; u < C->nupd && u < 2u; u++) lead += h2he_int_len(C->upd[u], 5);
  __syncthreads();
  if (tid == 0) {
    uint32_t cur_max = F->cur_max, size = F->size, cnt = F->cnt, evicted = 0;
    const uint32_t ins = F->ins;
    if (nblk)
      for (uint32_t u = 0; u < C->nupd && u < 2u; u++) {  // (the evictions come first)
        cur_max = C->upd[u];
        while (cnt && size > cur_max) {
          const uint32_t slot = (ins - cnt) & mask;
          size -= 32u + s_nl[slot] + s_vl[slot];
          cnt--;
          evicted++;
        }
      }
    s_cur_max = cur_max;
    s_size = size;
    s_cnt = cnt;
    s_ins = ins;
    s_inserted = 0;
    s_evicted = evicted;
  }
  __syncthreads();
  // ---- the occurrences, one a thread
  uint64_t run = lead, list = 0;  // (uniform) block bytes and header-list bytes so far
  uint32_t kb = 0;                // (uniform) a block at or in front of the step's first occurrence
  for (uint64_t o0 = 0; o0 < nwalk; o0 += H2HE_CHUNK) {  // (uniform)
    const uint64_t i = o0 + tid;
    const bool active = i < nwalk;
    for (uint32_t j = tid; j <= H2HE_CHUNK; j += H2HE_THREADS) s_occ0[j] = kb + j <= lim ? C->blks[kb + j].occ0 : ~0ull;
    __syncthreads();
    uint32_t blk = 0, hint = 0, nl = 0, vl = 0, sfull = 0, sname = 0, bad = 0;
    h2he_rec r = {0, 0, 0, 0, 0, {0, 0, 0}};
    h2hp_field_out f = {0, 0, 0, 0};
    const uint8_t* name = nullptr;
    const uint8_t* value = nullptr;
    uint32_t my_full = H2HE_NONE, my_name = H2HE_NONE;  // the newest matching entries: their insertion numbers
    uint32_t my_ins = s_ins;                            // insertions in front of this occurrence
    uint32_t t_cnt = 0;                                 // entries this occurrence looks through
    // what it still looks for: 1 a full match, 2 a name match; 4 it is a good occurrence; 8 it has inserted
    uint32_t st = 0;
    if (active) {
      uint32_t lo = 0, hi = H2HE_CHUNK + 1u;  // the block: the last one with occ0 <= i, among the staged ones ...
      while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s_occ0[mid] <= i) lo = mid;
        else hi = mid;
      }
      const bool staged = lo < H2HE_CHUNK;
      blk = kb + lo;
      lo = blk;
      hi = staged ? blk + 1u : lim;  // ... or behind them (a run of empty blocks)
      while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (C->blks[mid].occ0 <= i) lo = mid;
        else hi = mid;
      }
      const uint64_t occ0 = staged ? s_occ0[lo - kb] : C->blks[lo].occ0;
      blk = lo;
      if (tid == H2HE_THREADS - 1u || i + 1u == nwalk) s_kb = blk;
      const uint64_t fi = (uint64_t)C->blocks[blk].first_field + (i - occ0);
      f = C->fields[fi];
      r = C->recs[fi];
      hint = (f.name_len >> 24) & 3u;
      nl = f.name_len & 0xffffffu;
      vl = f.value_len;
      bad = r.st >> 16;
      sfull = r.st & 0xffu;
      sname = (r.st >> 8) & 0xffu;
      name = C->strings + f.name_off;
      value = C->strings + f.value_off;
      if (bad) atomicMin(&s_badocc, (uint32_t)i);
      else st = 4u | ((hint != 3u && !sfull) ? 1u : 0u) | (sname ? 0u : 2u);
      if (st & 3u) t_cnt = s_cnt;
    }
    // the table in front of the step, newest first
    for (uint32_t q = 0; q < t_cnt; q++) {
      const uint32_t e = my_ins - 1u - q, slot = e & mask;
      if (s_hn[slot] != r.hn || s_nl[slot] != nl) continue;
      const uint32_t full = (st & 1u) && s_hf[slot] == r.hf && s_vl[slot] == vl ? 1u : 0u;
      if (!full && !(st & 2u)) continue;
      const bool fresh = (int32_t)(e - ins0) >= 0;
      if (!h2he_same(F, C, fresh, s_ns[slot], name, nl)) continue;
      if (st & 2u) {
        my_name = e;
        st &= ~2u;
      }
      if (full && h2he_same(F, C, fresh, s_vs[slot], value, vl)) {
        my_full = e;
        st &= ~1u;
      }
      if (!(st & 3u)) break;
    }
    // the occurrences that insert, in wire order, one a round
    for (;;) {
      if (tid == 0) s_p = H2HE_CHUNK;
      __syncthreads();
      if ((st & 12u) == 4u && hint < 2u && !sfull && my_full == H2HE_NONE) atomicMin(&s_p, tid);
      __syncthreads();
      const uint32_t p = s_p;
      if (p == H2HE_CHUNK) break;  // (uniform)
      if (tid == p) {  // (its name reference stands: resolved in front of the evictions, RFC 7541 4.4)
        st |= 8u;
        uint32_t size = s_size, cnt = s_cnt, ins = s_ins, evicted = s_evicted;
        const uint32_t cur_max = s_cur_max;
        const uint64_t need = 32ull + nl + vl;
        while (cnt && (uint64_t)size + need > cur_max) {
          const uint32_t slot = (ins - cnt) & mask;
          size -= 32u + s_nl[slot] + s_vl[slot];
          cnt--;
          evicted++;
        }
        s_new = H2HE_NONE;
        if (need <= cur_max) {
          const uint32_t slot = ins & mask;
          s_hn[slot] = r.hn;
          s_hf[slot] = r.hf;
          s_nl[slot] = nl;
          s_vl[slot] = vl;
          s_ns[slot] = f.name_off;
          s_vs[slot] = f.value_off;
          s_new = ins;
          ins++;
          cnt++;
          size += (uint32_t)need;
          s_inserted++;
        }
        s_size = size;
        s_cnt = cnt;
        s_ins = ins;
        s_evicted = evicted;
      }
      __syncthreads();
      if ((st & 4u) && tid > p) {
        const uint32_t oldest = s_ins - s_cnt, e = s_new, slot = e & mask;
        // an entry that is gone leaves no older match either
        if (my_full != H2HE_NONE && (int32_t)(my_full - oldest) < 0) my_full = H2HE_NONE;
        if (my_name != H2HE_NONE && (int32_t)(my_name - oldest) < 0) my_name = H2HE_NONE;
        my_ins = s_ins;
        // the new entry is one more candidate, and the newest
        if (e != H2HE_NONE && s_hn[slot] == r.hn && s_nl[slot] == nl && h2he_same(F, C, true, s_ns[slot], name, nl)) {
          if (!sname) my_name = e;
          if (hint != 3u && !sfull && s_hf[slot] == r.hf && s_vl[slot] == vl && h2he_same(F, C, true, s_vs[slot], value, vl)) my_full = e;
        }
      }
    }
    const bool inserts = (st & 8u) != 0;
    // representation, index, size
    uint32_t rep = 0, idx = 0, sz = 0;
    if (active && !bad) {
      if (hint != 3u && !inserts && (sfull || my_full != H2HE_NONE)) {
        idx = sfull ? sfull : 62u + (my_ins - 1u - my_full);
        sz = h2he_int_len(idx, 7);
      } else {
        rep = hint < 2u ? 1u : hint;
        idx = sname ? sname : my_name != H2HE_NONE ? 62u + (my_ins - 1u - my_name) : 0u;
        sz = h2he_int_len(idx, rep == 1u ? 6 : 4) + (idx ? 0u : h2he_str_len(r.nenc)) + h2he_str_len(r.venc);
      }
    }
    uint64_t tot, tot_list;
    const uint64_t x = run + block_excl_scan((uint64_t)sz, s_wave, &tot);
    block_excl_scan(active && !bad ? (uint64_t)nl + vl : 0ull, s_wave, &tot_list);
    if (active) C->occs[i] = h2he_occ{x, idx | (rep << 28) | (bad ? 0x80000000u : 0u), blk};
    run += tot;
    list += tot_list;
    kb = s_kb;  // (behind the scans' barriers)
  }
  __syncthreads();
  // ---- bad input: the first block with a fault
  {
    uint32_t bad = s_badblk, code = 0;
    if (s_badocc != H2HE_NONE) {
      const uint32_t b = C->occs[s_badocc].blk;
      if (b < bad) {
        bad = b;
        const uint64_t fi = (uint64_t)C->blocks[b].first_field + (s_badocc - C->blks[b].occ0);
        code = C->recs[fi].st >> 16;
      }
    }
    if (bad != H2HE_NONE) {  // (uniform)
      if (tid == 0) {
        if (!code) {
          const h2hp_block_out B = C->blocks[bad];
          code = (uint64_t)B.first_field + B.nfields > C->nfields ? H2HE_E_FIELD_RANGE : H2HE_E_STREAM;
        }
        for (int k = 0; k < 8; k++) R[k] = 0;
        R[H2HE_TABLE] = F->size;
        R[H2HE_FLAGS] = (uint64_t)H2HE_F_BAD_INPUT | ((uint64_t)code << 8) | ((uint64_t)bad << 32);
        *N = 0;
      }
      return;
    }
  }
  // ---- the blocks: their bytes, their frames, their place in the wire arena
  uint64_t wire = 0, frames = 0;
  const uint32_t max_frame = C->max_frame;
  for (uint32_t k0 = 0; k0 < nblk; k0 += H2HE_THREADS) {  // (uniform)
    const uint32_t k = k0 + tid;
    uint64_t ps = 0, wb = 0, nfr = 0;
    if (k < nblk) {
      const uint64_t a = C->blks[k].occ0, b = C->blks[k + 1u].occ0;
      ps = k == 0 ? 0ull : a < nwalk ? C->occs[a].pos : run;  // (block 0 begins with the size updates)
      const uint64_t pe = k + 1u == nblk ? run : b < nwalk ? C->occs[b].pos : run;
      const uint64_t len = pe - ps;
      nfr = len ? (len + max_frame - 1u) / max_frame : 1ull;
      wb = len + 9ull * nfr;
      if (wb > 0xffffffffull) atomicMin(&s_big, k);
    }
    uint64_t tot_w, tot_f;
    const uint64_t x = wire + block_excl_scan(wb, s_wave, &tot_w);
    block_excl_scan(nfr, s_wave, &tot_f);
    if (k < nblk) {
      h2he_blk* o = &C->blks[k];
      o->pstart = ps;
      o->woff = x;
      o->len = (uint32_t)wb;
      o->nframes = (uint32_t)nfr;
    }
    wire += tot_w;
    frames += tot_f;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 0; k < 8; k++) R[k] = 0;
    *N = 0;
    if (s_big != H2HE_NONE) {
      R[H2HE_TABLE] = F->size;
      R[H2HE_FLAGS] = (uint64_t)H2HE_F_BAD_INPUT | ((uint64_t)H2HE_E_BLOCK_TOO_LARGE << 8) | ((uint64_t)s_big << 32);
    } else {
      const bool over = wire > C->wire_cap || nblk > C->bw_cap;
      R[H2HE_BLOCKS] = nblk;
      R[H2HE_FRAMES] = frames;
      R[H2HE_WIRE] = wire;
      R[H2HE_INSERTED] = s_inserted;
      R[H2HE_EVICTED] = s_evicted;
      R[H2HE_TABLE] = s_size;
      R[H2HE_OVERFLOW] = over ? H2HE_OVER_CAPS : 0;
      if (!over) {
        // the entries this call inserted and that live get their place in the byte ring, behind the older ones
        const uint32_t ins = s_ins, cnt = s_cnt;
        const uint32_t fresh = ins - ins0 < cnt ? ins - ins0 : cnt;
        uint32_t head = F->ring_head, nj = 0;
        for (uint32_t q = 0; q < fresh; q++) {
          const uint32_t slot = (ins - fresh + q) & mask;
          F->jobs[nj++] = h2he_job{s_ns[slot], s_vs[slot], head, s_nl[slot], s_vl[slot], 0};
          s_ns[slot] = head;
          head = (head + s_nl[slot] + s_vl[slot]) & (H2HP_BYTES - 1u);
        }
        F->njobs = nj;
        F->ring_head = head;
        F->cur_max = s_cur_max;
        F->size = s_size;
        F->cnt = cnt;
        F->ins = ins;
        F->st_calls++;
        F->st_blocks += nblk;
        F->st_fields += nwalk;
        F->st_list += list;
        F->st_wire += wire;
        F->st_inserted += s_inserted;
        F->st_evicted += s_evicted;
        *N = nwalk;
        F->go = 1;
        s_commit = 1;
      }
    }
  }
  __syncthreads();
  if (s_commit)
    for (uint32_t i = tid; i < H2HP_RING; i += H2HE_THREADS) {
      F->r_hn[i] = s_hn[i];
      F->r_hf[i] = s_hf[i];
      F->r_nl[i] = s_nl[i];
      F->r_vl[i] = s_vl[i];
      F->r_src[i] = s_ns[i];
    }

#elif H2HE_STAGE == 3  // k_h2_hpenc_emit: a lane per occurrence, a lane per block
  __shared__ uint32_t s_code[256];
  __shared__ uint8_t s_bits[256];
  if (!F->go) return;  // (uniform) nothing half-written
  const uint32_t tid = threadIdx.x;
  s_code[tid] = F->huff_code[tid];
  s_bits[tid] = F->huff_bits[tid];
  __syncthreads();
  const uint64_t gtid = (uint64_t)(H2HE_BLK) * H2HE_THREADS + tid, gsz = (uint64_t)(H2HE_NBLK) * H2HE_THREADS;
  const uint64_t nocc = *N < C->occs_cap ? *N : C->occs_cap;
  const uint32_t max_frame = C->max_frame, nblk = (uint32_t)C->nblocks;
  for (uint64_t i = gtid; i < nocc; i += gsz) {
    const h2he_occ o = C->occs[i];
    const h2he_blk B = C->blks[o.blk];
    const uint64_t fi = (uint64_t)C->blocks[o.blk].first_field + (i - B.occ0);
    const h2hp_field_out f = C->fields[fi];
    const h2he_rec r = C->recs[fi];
    const uint32_t rep = (o.w >> 28) & 3u, idx = o.w & 0xffffffu;
    h2he_out w = h2he_open(C->wire + B.woff, B.len, o.pos - B.pstart, max_frame);
    if (rep == 0) {
      h2he_put_int(w, idx, 7, 0x80u);
      continue;
    }
    h2he_put_int(w, idx, rep == 1u ? 6 : 4, rep == 1u ? 0x40u : rep == 3u ? 0x10u : 0u);
    if (!idx) h2he_put_str(w, C->strings + f.name_off, f.name_len & 0xffffffu, r.nenc, s_code, s_bits);
    h2he_put_str(w, C->strings + f.value_off, f.value_len, r.venc, s_code, s_bits);
  }
  for (uint64_t k = gtid; k < nblk; k += gsz) {
    const h2he_blk B = C->blks[k];
    const h2hp_block_out in = C->blocks[k];
    uint8_t* base = C->wire + B.woff;
    const uint32_t payload = B.len - 9u * B.nframes;
    for (uint32_t j = 0; j < B.nframes; j++) {
      uint8_t* h = base + (uint64_t)j * (max_frame + 9ull);
      const uint32_t left = payload - j * max_frame, n = left < max_frame ? left : max_frame;
      h[0] = (uint8_t)(n >> 16);
      h[1] = (uint8_t)(n >> 8);
      h[2] = (uint8_t)n;
      h[3] = j ? (uint8_t)FT_CONTINUATION : (uint8_t)FT_HEADERS;
      h[4] = (uint8_t)((j + 1u == B.nframes ? 0x4u : 0u) | (j == 0 ? (in.flags & 1u) : 0u));
      h[5] = (uint8_t)(in.stream >> 24);
      h[6] = (uint8_t)(in.stream >> 16);
      h[7] = (uint8_t)(in.stream >> 8);
      h[8] = (uint8_t)in.stream;
    }
    if (k == 0) {
      h2he_out w = h2he_open(base, B.len, 0, max_frame);
      for (uint32_t u = 0; u < C->nupd && u < 2u; u++) h2he_put_int(w, C->upd[u], 5, 0x20u);
    }
    C->bw[k] = h2he_wire_out{B.woff, B.len, B.nframes};
  }

#elif H2HE_STAGE == 4  // k_h2_hpenc_commit: the inserted entries' strings into the byte ring
  if (!F->go) return;  // (uniform) nothing is committed
  const uint64_t gtid = (uint64_t)(H2HE_BLK) * H2HE_THREADS + threadIdx.x, gsz = (uint64_t)(H2HE_NBLK) * H2HE_THREADS;
  const uint32_t nj = F->njobs < H2HP_RING ? F->njobs : H2HP_RING;
  for (uint64_t j = gtid; j < nj; j += gsz) {
    const h2he_job job = F->jobs[j];
    const uint8_t* name = C->strings + job.name_src;
    const uint8_t* value = C->strings + job.value_src;
    for (uint32_t k = 0; k < job.name_len; k++) F->bytes[(job.dst + k) & (H2HP_BYTES - 1u)] = name[k];
    for (uint32_t k = 0; k < job.value_len; k++) F->bytes[(job.dst + job.name_len + k) & (H2HP_BYTES - 1u)] = value[k];
  }
#endif
