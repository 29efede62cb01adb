// The bodies of the metadata reader's stages as source text, included by the single-call kernels (k_h2_meta_*: H2M_BLK =
// blockIdx.x, H2M_NBLK = H2M_GRID, H2M_LINKS 0) and by the kernels over a table of links (k_h2_links_meta_*: a link's
// share of the grid, H2M_LINKS 1), csrc/grdma_h2_meta.h.  H2M_STAGE selects the stage.  A stage expects in scope, as the
// including kernel names them:
//   h2m_dev* F           the reader: the constants (method table, keys, accept, rej_first, rej_n) and the counters
//   const h2m_call* C    the call's words (&F->c in the single kernels, the item's words of the batch block over links)
//   h2m_wg* W            the H2M_NBLK counts of the workgroups that share the call (stages 2 and 3)
//   uint64_t* R          the eight result words the host reads (stage 3)
//   tab, nlinks          over links, stage 3: the table, for the one count of the reader's counters
// (Source text rather than device functions, as csrc/grdma_h2_hpenc_stage.inc.)
#if H2M_STAGE == 1  // k_h2_meta_fields: a lane per field of the field table
  __shared__ uint32_t s_kw[H2M_NKEYS][H2M_KEY_WORDS];  // the known keys as h2m_load4 packs a name
  __shared__ uint32_t s_kl[H2M_NKEYS];                 // their lengths
  const uint32_t tid = threadIdx.x;
  if (tid < H2M_NKEYS * H2M_KEY_WORDS) {
    const uint32_t q = tid / H2M_KEY_WORDS, j = tid % H2M_KEY_WORDS, o = F->key_off[q], ln = F->key_off[q + 1u] - o;
    uint32_t w = 0;
    for (uint32_t k = 4u * j; k < ln && k < 4u * j + 4u; k++) w |= (uint32_t)F->key_bytes[o + k] << (8u * (k & 3u));
    s_kw[q][j] = w;
    if (j == 0) s_kl[q] = ln;
  }
  __syncthreads();
  const uint64_t nf = C->nfields < C->recs_cap ? C->nfields : C->recs_cap, ns = C->strings_bytes;
  const uint64_t gsz = (uint64_t)(H2M_NBLK) * H2M_THREADS;
  for (uint64_t i = (uint64_t)(H2M_BLK) * H2M_THREADS + tid; i < nf; i += gsz) {
    const h2hp_field_out f = C->fields[i];
    const uint32_t nl = f.name_len & 0xffffffu, vl = f.value_len;
    h2m_rec r = {0, 0, 0, 0};
    if ((uint64_t)f.name_off + nl > ns || (uint64_t)f.value_off + vl > ns) {
      r.w = H2M_R_INPUT;
      C->recs[i] = r;
      continue;
    }
    const uint8_t* name = C->strings + f.name_off;
    const uint8_t* value = C->strings + f.value_off;
    // the name: a-z 0-9 - _ . and a ':' in front; its first 20 bytes packed
    uint32_t bad = nl == 0, n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0;
    for (uint32_t k = 0; k < nl; k += 4u) {
      const uint32_t w = h2m_load4(name, k, nl);
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t b = (w >> (8u * j)) & 0xffu;
        const bool ok = (b - 0x61u < 26u) || (b - 0x30u < 10u) || b == 0x2du || b == 0x5fu || b == 0x2eu || (k + j == 0 && b == 0x3au);
        bad |= k + j < nl && !ok;
      }
      if (k == 0) n0 = w;
      else if (k == 4u) n1 = w;
      else if (k == 8u) n2 = w;
      else if (k == 12u) n3 = w;
      else if (k == 16u) n4 = w;
    }
    const bool pseudo = nl && (n0 & 0xffu) == 0x3au;
    uint32_t key = 0;
    if (nl <= 4u * H2M_KEY_WORDS)
#pragma nounroll  // (unrolled, the seventeen bodies keep a mask pair each and the kernel spills scalar registers)
      for (uint32_t q = 0; q < H2M_NKEYS; q++)
        if (s_kl[q] == nl && !((n0 ^ s_kw[q][0]) | (n1 ^ s_kw[q][1]) | (n2 ^ s_kw[q][2]) | (n3 ^ s_kw[q][3]) | (n4 ^ s_kw[q][4]))) key = q + 1u;
    bad |= pseudo && !(key >= H2M_K_METHOD && key <= H2M_K_STATUS);
    bad |= key >= H2M_KEY_CONNECTION;
    // the value: visible ASCII unless the name ends in -bin; its first 17 bytes packed (every value a key calls for
    // fits) and its hash (FNV-1a: what a :path is looked up by)
    const bool bin = nl >= 4u && h2m_load4(name, nl - 4u, nl) == H2M_LIT4('-', 'b', 'i', 'n');
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0, b16 = 0, out = 0, hash = 0x811c9dc5u;
    for (uint32_t k = 0; k < vl; k += 4u) {
      const uint32_t w = h2m_load4(value, k, vl);
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t b = (w >> (8u * j)) & 0xffu;
        if (k + j < vl) {
          out |= b - 0x20u > 0x5eu;
          hash = h2he_fnv(hash, b);
        }
      }
      if (k == 0) w0 = w;
      else if (k == 4u) w1 = w;
      else if (k == 8u) w2 = w;
      else if (k == 12u) w3 = w;
      else if (k == 16u) b16 = w & 0xffu;
    }
    const uint64_t v0 = (uint64_t)w0 | (uint64_t)w1 << 32;
    bad |= out && !bin;
    bool good = false;
    if (key == H2M_K_METHOD) {
      good = vl == 4u && w0 == H2M_LIT4('P', 'O', 'S', 'T');
    } else if (key == H2M_K_SCHEME) {
      good = w0 == H2M_LIT4('h', 't', 't', 'p') && (vl == 4u || (vl == 5u && w1 == (uint32_t)'s'));
    } else if (key == H2M_K_PATH) {
      good = vl != 0;
      r.lo = H2M_NONE;
      if (vl - 1u < 1024u) {
        for (uint32_t at = hash & F->slot_mask;; at = (at + 1u) & F->slot_mask) {  // (at most half the slots are taken)
          const h2m_slot s = F->slots[at];
          if (!s.len) break;
          if (s.hash == hash && s.len == vl && h2he_eq(F->paths, s.off, 0xffffffffu, value, vl)) {
            r.lo = s.id;
            break;
          }
        }
      }
    } else if (key == H2M_K_STATUS) {
      good = vl == 3u && h2m_number(v0, 3, &r.lo);
    } else if (key == H2M_K_GRPC_STATUS) {
      good = vl - 1u < 3u && h2m_number(v0, vl, &r.lo);
    } else if (key == H2M_K_CONTENT_TYPE) {  // application/grpc, alone or with '+' or ';' behind it
      good = vl >= 16u && H2M_IS8('a', 'p', 'p', 'l', 'i', 'c', 'a', 't') && w2 == H2M_LIT4('i', 'o', 'n', '/') && w3 == H2M_LIT4('g', 'r', 'p', 'c') &&
             (vl == 16u || b16 == 0x2bu || b16 == 0x3bu);
    } else if (key == H2M_K_TE) {
      good = vl == 8u && H2M_IS8('t', 'r', 'a', 'i', 'l', 'e', 'r', 's');
      bad |= !good;
    } else if (key == H2M_K_ENCODING) {
      r.lo = (vl == 8u && H2M_IS8('i', 'd', 'e', 'n', 't', 'i', 't', 'y')) ? 0u : (vl == 4u && w0 == H2M_LIT4('g', 'z', 'i', 'p')) ? 1u :
             (vl == 7u && H2M_IS8('d', 'e', 'f', 'l', 'a', 't', 'e', 0)) ? 2u : 255u;
    } else if (key == H2M_K_TIMEOUT) {  // 1 to 8 digits and a unit
      uint32_t n = 0;
      if (vl - 2u < 8u && h2m_number(v0, vl - 1u, &n)) {
        const uint32_t u = vl == 9u ? w2 & 0xffu : (uint32_t)(v0 >> (8u * (vl - 1u))) & 0xffu;
        // the unit in two 32-bit factors: seconds, and nanoseconds per second or its part
        const uint32_t secs = u == 0x48u ? 3600u : u == 0x4du ? 60u : 1u;
        const uint32_t part = (u == 0x48u || u == 0x4du || u == 0x53u) ? 1000000000u : u == 0x6du ? 1000000u : u == 0x75u ? 1000u : u == 0x6eu ? 1u : 0u;
        if (part) {
          // (99999999H passes 2^64: compared first.  Only hours can pass 2^63 - 1 with eight digits.)
          static_assert(0x7fffffffffffffffull / 3600000000000ull == 2562047ull && 0x7fffffffffffffffull / 60000000000ull > 99999999ull,
                        "the one unit that saturates");
          const uint64_t ns64 = (u == 0x48u && n > 2562047u) ? 0x7fffffffffffffffull : (uint64_t)n * secs * part;
          good = true;
          r.lo = (uint32_t)ns64;
          r.hi = (uint32_t)(ns64 >> 32);
        }
      }
    }
    r.w = key | (bad ? H2M_R_BAD : 0u) | (good ? H2M_R_GOOD : 0u) | (pseudo ? H2M_R_PSEUDO : 0u);
    C->recs[i] = r;
  }
#elif H2M_STAGE == 2  // k_h2_meta_blocks: a wave per block, a workgroup a contiguous run of blocks
  __shared__ uint32_t s_cnt[H2M_BLK_THREADS / 64][6];
  __shared__ uint64_t s_bad[H2M_BLK_THREADS / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t before = (1ull << lane) - 1ull;
  uint64_t b0, b1;
  h2m_run(C->nblocks < C->mrecs_cap ? C->nblocks : C->mrecs_cap, H2M_BLK, H2M_NBLK, &b0, &b1);
  uint32_t n_rej = 0, n_req = 0, n_resp = 0, n_trail = 0, n_malformed = 0;
  uint64_t first_bad = ~0ull;
  for (uint64_t blk = b0 + wave; blk < b1; blk += H2M_BLK_THREADS / 64) {  // (uniform in the wave)
    const h2hp_block_out B = C->blocks[blk];
    uint32_t err = 0;
    if ((uint64_t)B.first_field + B.nfields > C->nfields || (uint64_t)B.first_field + B.nfields > C->recs_cap) err = H2M_E_FIELD_RANGE;
    else if (B.stream == 0 || B.stream > 0x7fffffffu) err = H2M_E_STREAM;
    // what the steps in front left: the keys seen (bit k), a regular field, the first fault, a :status that is no number
    uint32_t seen = 0, regular = 0, bad_field = H2M_NONE, status_late = H2M_NONE, ncustom = 0;
    // the first occurrence of a key: its field (the four the record names), whether its value is good (bit k), its number
    uint32_t at_path = H2M_NONE, at_authority = H2M_NONE, at_message = H2M_NONE, at_status = H2M_NONE, goodm = 0;
    uint32_t v_path = H2M_NONE, v_status = 0, v_enc = 0, v_grpc = 0, t_lo = 0, t_hi = 0;
    for (uint32_t s = 0; s < B.nfields && !err; s += 64u) {
      const bool have = s + lane < B.nfields;
      h2m_rec r = {0xffu, 0, 0, 0};
      if (have) r = C->recs[(uint64_t)B.first_field + s + lane];
      const uint32_t key = r.w & 0xffu;
      if (__ballot(have && (r.w & H2M_R_INPUT))) {
        err = H2M_E_STRING;
        break;
      }
      const bool pseudo = have && (r.w & H2M_R_PSEUDO);
      const uint64_t regm = __ballot(have && !pseudo);
      uint64_t mine = 0, reqm = 0, m5 = 0;
      uint32_t now = 0;
#pragma unroll
      for (uint32_t k = 1; k <= H2M_K_LAST; k++) {
        const uint64_t mk = __ballot(key == k);
        if (k <= H2M_K_STATUS && key == k) mine = mk;
        if (k < H2M_K_STATUS) reqm |= mk;
        if (k == H2M_K_STATUS) m5 = mk;
        if (mk) now |= 1u << k;
        if (mk && !((seen >> k) & 1u)) {  // the first occurrence wins
          const uint32_t src = (uint32_t)__builtin_ctzll(mk), field = B.first_field + s + src;
          if (k != H2M_K_AUTHORITY && k != H2M_K_ACCEPT && k != H2M_K_MESSAGE) goodm |= ((h2m_from(r.w, src) >> 9) & 1u) << k;
          if (k == H2M_K_PATH) at_path = field, v_path = h2m_from(r.lo, src);
          if (k == H2M_K_AUTHORITY) at_authority = field;
          if (k == H2M_K_MESSAGE) at_message = field;
          if (k == H2M_K_STATUS) at_status = field, v_status = h2m_from(r.lo, src);
          if (k == H2M_K_ENCODING) v_enc = h2m_from(r.lo, src);
          if (k == H2M_K_GRPC_STATUS) v_grpc = h2m_from(r.lo, src);
          if (k == H2M_K_TIMEOUT) t_lo = h2m_from(r.lo, src), t_hi = h2m_from(r.hi, src);
        }
      }
      ncustom += (uint32_t)__builtin_popcountll(__ballot(have && key == 0));
      bool fault = have && (r.w & H2M_R_BAD);
      if (pseudo) fault |= regular || (regm & before);
      if (key >= H2M_K_METHOD && key <= H2M_K_STATUS) {
        fault |= ((seen >> key) & 1u) || (mine & before);
        if (key == H2M_K_STATUS) fault |= (seen & 0x1eu) || (reqm & before);
        else fault |= ((seen >> H2M_K_STATUS) & 1u) || (m5 & before);
        if (key == H2M_K_SCHEME || key == H2M_K_PATH) fault |= !(r.w & H2M_R_GOOD);
      }
      const uint64_t fm = __ballot(fault);
      if (fm && bad_field == H2M_NONE) bad_field = B.first_field + s + (uint32_t)__builtin_ctzll(fm);
      if (m5 && !((seen >> H2M_K_STATUS) & 1u) && !((goodm >> H2M_K_STATUS) & 1u)) status_late = at_status;
      seen |= now;
      regular |= regm != 0;
    }
    if (err) {
      if (first_bad == ~0ull) first_bad = blk << 8 | err;
      continue;
    }
    // the record (every lane holds the same values; lane 0 writes)
    const bool is_req = seen & 0x1eu, has_status = (seen >> H2M_K_STATUS) & 1u;
    const uint32_t kind = is_req ? H2M_REQUEST : has_status ? H2M_RESPONSE : H2M_IS_TRAILERS;
    if (kind == H2M_RESPONSE && status_late < bad_field) bad_field = status_late;
    const bool malformed = bad_field != H2M_NONE || (is_req && (seen & 0xeu) != 0xeu);
#define H2M_HAS(k) ((seen >> (k)) & 1u)
#define H2M_GOOD(k) (H2M_HAS(k) && ((goodm >> (k)) & 1u))
    const uint32_t enc = H2M_HAS(H2M_K_ENCODING) ? v_enc : 0u;
    const uint32_t method = v_path;
    const uint32_t http_status = H2M_GOOD(H2M_K_STATUS) ? v_status : H2M_NONE;
    const uint32_t end = B.flags & 1u;
    uint32_t verdict = H2M_OK;
    if (malformed) verdict = H2M_V_MALFORMED;
    else if (is_req && !H2M_GOOD(H2M_K_METHOD)) verdict = H2M_BAD_METHOD;
    else if (kind != H2M_IS_TRAILERS && !H2M_GOOD(H2M_K_CONTENT_TYPE)) verdict = H2M_BAD_CONTENT_TYPE;
    else if (is_req && !H2M_HAS(H2M_K_TE)) verdict = H2M_BAD_TE;
    else if (H2M_HAS(H2M_K_TIMEOUT) && !H2M_GOOD(H2M_K_TIMEOUT)) verdict = H2M_BAD_TIMEOUT;
    else if (is_req && method == H2M_NONE) verdict = H2M_UNIMPLEMENTED;
    else if (is_req && (enc > 2u || !((F->accept >> enc) & 1u))) verdict = H2M_BAD_ENCODING;
    else if (kind == H2M_RESPONSE && http_status != 200u) verdict = H2M_HTTP_STATUS;
    else if (end && !is_req && !H2M_HAS(H2M_K_GRPC_STATUS)) verdict = H2M_NO_STATUS;
    else if (H2M_HAS(H2M_K_GRPC_STATUS) && !H2M_GOOD(H2M_K_GRPC_STATUS)) verdict = H2M_BAD_GRPC_STATUS;
    const uint32_t has_timeout = H2M_GOOD(H2M_K_TIMEOUT);
    const uint32_t flags = (has_timeout ? H2M_HAS_TIMEOUT : 0u) | (end ? H2M_END_STREAM : 0u) |
                           (H2M_HAS(H2M_K_GRPC_STATUS) ? H2M_HAS_GRPC_STATUS : 0u) | (H2M_HAS(H2M_K_MESSAGE) ? H2M_HAS_MESSAGE : 0u);
    const h2m_meta_out m = {B.stream, kind | verdict << 8 | enc << 16 | flags << 24, method, http_status,
                            H2M_GOOD(H2M_K_GRPC_STATUS) ? v_grpc : H2M_NONE, has_timeout ? t_lo : 0u,
                            has_timeout ? t_hi : 0u, at_path, at_authority, at_message, ncustom, bad_field};
#undef H2M_GOOD
#undef H2M_HAS
    if (lane == 0) C->mrecs[blk] = m;
    n_req += kind == H2M_REQUEST;
    n_resp += kind == H2M_RESPONSE;
    n_trail += kind == H2M_IS_TRAILERS;
    n_malformed += malformed;
    n_rej += h2m_rejected(m.word);
  }
  if (lane == 0) {
    s_cnt[wave][0] = n_rej;
    s_cnt[wave][1] = n_req;
    s_cnt[wave][2] = n_resp;
    s_cnt[wave][3] = n_trail;
    s_cnt[wave][4] = n_malformed;
    s_bad[wave] = first_bad;
  }
  __syncthreads();
  if (tid == 0) {
    h2m_wg g = {0, 0, 0, 0, 0, 0, ~0ull};
    for (uint32_t w = 0; w < H2M_BLK_THREADS / 64; w++) {
      g.rej += s_cnt[w][0];
      g.req += s_cnt[w][1];
      g.resp += s_cnt[w][2];
      g.trail += s_cnt[w][3];
      g.malformed += s_cnt[w][4];
      if (s_bad[w] < g.bad) g.bad = s_bad[w];
    }
    W[H2M_BLK] = g;
  }
#elif H2M_STAGE == 3  // k_h2_meta_emit: the records and the rejection blocks out, the result block, the counters
  __shared__ uint64_t s_wave[H2M_THREADS / 64];
  const uint32_t tid = threadIdx.x;
#if H2M_LINKS
  // the reader's counters, once for the call: workgroup 0 of the launch, a thread per link.  A link's counts stand since
  // the blocks stage ended; it is read where its own workgroups (below) find neither bad input nor a cap too small.
  __shared__ uint64_t s_tot[H2M_THREADS / 64][7];
  static_assert(H2M_LINKS_MAX <= H2M_THREADS, "a thread per link");
  if (blockIdx.x == 0) {  // (uniform)
    uint64_t t_read = 0, t_nb = 0, t_req = 0, t_resp = 0, t_trail = 0, t_rej = 0, t_malformed = 0;
    if (tid < nlinks) {
      const h2m_call* const c = H2M_ENTRY(tab, tid).call;
      const h2m_wg* const w = H2M_ENTRY(tab, tid).wg;
      uint64_t rej = 0, req = 0, resp = 0, trail = 0, malformed = 0, bad = ~0ull;
#pragma unroll
      for (uint32_t k = 0; k < H2M_LINK_GRID; k++) {
        const h2m_wg g = w[k];
        rej += g.rej;
        req += g.req;
        resp += g.resp;
        trail += g.trail;
        malformed += g.malformed;
        if (g.bad < bad) bad = g.bad;
      }
      const uint64_t nb = c->nblocks;
      if (bad == ~0ull && nb <= c->mrecs_cap && nb <= c->meta_cap && rej <= c->reject_cap)
        t_read = 1, t_nb = nb, t_req = req, t_resp = resp, t_trail = trail, t_rej = rej, t_malformed = malformed;
    }
    for (int d = 32; d >= 1; d >>= 1) {
      t_read += __shfl_xor(t_read, d, 64);
      t_nb += __shfl_xor(t_nb, d, 64);
      t_req += __shfl_xor(t_req, d, 64);
      t_resp += __shfl_xor(t_resp, d, 64);
      t_trail += __shfl_xor(t_trail, d, 64);
      t_rej += __shfl_xor(t_rej, d, 64);
      t_malformed += __shfl_xor(t_malformed, d, 64);
    }
    if ((tid & 63u) == 0) {
      uint64_t* const t = s_tot[tid >> 6];
      t[0] = t_read, t[1] = t_nb, t[2] = t_req, t[3] = t_resp, t[4] = t_trail, t[5] = t_rej, t[6] = t_malformed;
    }
    __syncthreads();
    if (tid < 7u) {  // (a thread per counter)
      uint64_t v = 0, any = 0;
      for (uint32_t k = 0; k < H2M_THREADS / 64; k++) v += s_tot[k][tid], any += s_tot[k][0];
      if (any) (&F->st_calls)[tid] += tid ? v : 1ull;  // (st_calls .. st_malformed, in this order; no link read: nothing moves)
    }
  }
#endif
  // the counts in front of this workgroup's run and the totals: a lane of wave 0 per workgroup of k_h2_meta_blocks (a
  // loop over them in every thread is 64 dependent scalar loads)
  __shared__ uint64_t s_sum[7];
  static_assert(H2M_NBLK <= 64, "a lane per workgroup");
  if (tid < 64u) {
    h2m_wg g = {0, 0, 0, 0, 0, 0, ~0ull};
    if (tid < H2M_NBLK) g = W[tid];
    const uint64_t incl = wave_incl_scan((uint64_t)g.rej, (int)tid);
    uint64_t a = (uint64_t)g.req | (uint64_t)g.resp << 32, b = (uint64_t)g.trail | (uint64_t)g.malformed << 32, worst = g.bad;
    for (int d = 32; d >= 1; d >>= 1) {  // (sums of counts of at most 2^32 - 2 blocks: no carry between the halves)
      a += __shfl_xor(a, d, 64);
      b += __shfl_xor(b, d, 64);
      const uint64_t o = __shfl_xor(worst, d, 64);
      if (o < worst) worst = o;
    }
    const uint64_t mine = __shfl(incl - g.rej, (int)(H2M_BLK), 64), all = __shfl(incl, 63, 64);
    if (tid == 0) {
      s_sum[0] = mine;
      s_sum[1] = all;
      s_sum[2] = a & 0xffffffffull;
      s_sum[3] = a >> 32;
      s_sum[4] = b & 0xffffffffull;
      s_sum[5] = b >> 32;
      s_sum[6] = worst;
    }
  }
  __syncthreads();
  const uint64_t rej0 = s_sum[0], rej = s_sum[1], req = s_sum[2], resp = s_sum[3], trail = s_sum[4], malformed = s_sum[5], bad = s_sum[6];
  const uint64_t nb = C->nblocks;
  const bool bad_input = bad != ~0ull || nb > C->mrecs_cap;  // (the host sizes the scratch: the second cannot be)
  const bool over = nb > C->meta_cap || rej > C->reject_cap;
  if (bad_input || over) {  // (uniform) the result block alone
    if (H2M_BLK == 0 && tid == 0) {
      for (int k = 0; k < 8; k++) R[k] = 0;
      if (bad_input) {
        R[H2M_FLAGS] = H2M_F_BAD_INPUT | (bad & 0xffu) << 8 | (bad >> 8) << 32;
      } else {
        R[H2M_BLOCKS] = nb;
        R[H2M_REQUESTS] = req;
        R[H2M_RESPONSES] = resp;
        R[H2M_TRAILERS] = trail;
        R[H2M_REJECTIONS] = rej;
        R[H2M_MALFORMED] = malformed;
        R[H2M_OVERFLOW] = 1;
      }
    }
    return;
  }
  uint64_t b0, b1;
  h2m_run(nb, H2M_BLK, H2M_NBLK, &b0, &b1);
  // the records: 48 bytes each, three 16-byte words (both tables are aligned)
  const u32x4* const src = reinterpret_cast<const u32x4*>(C->mrecs);
  u32x4* const dst = reinterpret_cast<u32x4*>(C->meta);
  for (uint64_t j = 3u * b0 + tid; j < 3u * b1; j += H2M_THREADS) dst[j] = src[j];
  // the rejection blocks, in input order
  uint64_t run = rej0;
  for (uint64_t k0 = b0; k0 < b1; k0 += H2M_THREADS) {  // (uniform: the scan's barriers)
    const uint64_t k = k0 + tid;
    uint32_t word = 0, stream = 0;
    if (k < b1) {
      word = C->mrecs[k].word;
      stream = C->mrecs[k].stream;
    }
    const bool mine = k < b1 && h2m_rejected(word);
    uint64_t tot;
    const uint64_t x = run + block_excl_scan(mine ? 1ull : 0ull, s_wave, &tot);
    if (mine) {
      const uint32_t verdict = (word >> 8) & 0xfu;
      const h2hp_block_out o = {stream, F->rej_first[verdict], F->rej_n[verdict], 1u};
      C->reject[x] = o;
    }
    run += tot;
  }
  if (H2M_BLK == 0 && tid == 0) {
    R[H2M_BLOCKS] = nb;
    R[H2M_REQUESTS] = req;
    R[H2M_RESPONSES] = resp;
    R[H2M_TRAILERS] = trail;
    R[H2M_REJECTIONS] = rej;
    R[H2M_MALFORMED] = malformed;
    R[H2M_FLAGS] = 0;
    R[H2M_OVERFLOW] = 0;
#if !H2M_LINKS  // (over links: the count in front, once for the call)
    F->st_calls += 1;
    F->st_blocks += nb;
    F->st_requests += req;
    F->st_responses += resp;
    F->st_trailers += trail;
    F->st_rejections += rej;
    F->st_malformed += malformed;
#endif
  }
#endif
