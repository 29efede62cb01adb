// The body of the reply's plan workgroup as source text, included by k_h2_reply_plan (the one workgroup of the call) and
// by k_h2_reply_plan_links (workgroup l is link l's one plan workgroup), csrc/grdma_h2_reply.h.  It expects `h2r_dev* R`
// in scope, as k_h2_reply_plan's parameter is.
// (Source text rather than a device function: csrc/grdma_h2_frame_group.inc records that a function is simplified on its
// own before it is inlined and that the kernel it was taken from then came out as other bytes; with included text
// tools/h2_isa_compare.py reports k_h2_reply_plan `same`.)
  __shared__ uint64_t s_wave[PLAN_THREADS / 64];
  const h2a_dev* A = R->src;
  const uint64_t tid = threadIdx.x;
  // (a call the assembler skipped left no descriptors; more than the tables hold: nothing is framed)
  const bool bad = A->skip != 0 || A->ndesc > A->desc_cap || A->ndesc > R->max_messages;
  const uint64_t nd = bad ? 0 : A->ndesc;
  const grdma_h2_rx_msg* desc = A->desc;
  grdma_h2_msg_dev* msgs = R->msgs;
  // 1. kept or dropped, the kept ones compacted in descriptor order
  uint64_t kept = 0, my_status = 0, my_unrouted = 0;
  for (uint64_t d0 = 0; d0 < nd; d0 += PLAN_THREADS) {
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
    const uint64_t x = block_excl_scan(keep, s_wave, &tot);
    if (keep) msgs[kept + x] = m;
    kept += tot;
  }
  uint64_t n_status, n_unrouted;
  block_excl_scan(my_status, s_wave, &n_status);
  block_excl_scan(my_unrouted, s_wave, &n_unrouted);
  __syncthreads();  // the compacted table is complete: sizes look at a message's neighbours
  // 2. sizes and positions over the compacted table (the loop of k_h2_frame_index)
  const uint32_t max_frame = R->max_frame;
  uint64_t base_sl = 0, base_hdr = 0, base_wire = 0;
  for (uint64_t m0 = 0; m0 < kept; m0 += PLAN_THREADS) {
    const uint64_t i = m0 + tid;
    uint64_t n_sl = 0, n_hdr = 0, n_wire = 0;
    uint32_t mode = 0;
    if (i < kept) h2_msg_size(msgs, i, max_frame, &n_sl, &n_hdr, &n_wire, &mode);
    uint64_t tot_sl, tot_hdr, tot_wire;
    const uint64_t x_sl = block_excl_scan(n_sl, s_wave, &tot_sl);
    const uint64_t x_hdr = block_excl_scan(n_hdr, s_wave, &tot_hdr);
    block_excl_scan(n_wire, s_wave, &tot_wire);
    if (i < kept) {
      grdma_h2_msg_pos q;
      q.sl = base_sl + x_sl;
      q.hdr = base_hdr + x_hdr;
      q.mode = mode;
      q.pad = 0;
      R->pos[i] = q;
    }
    base_sl += tot_sl;
    base_hdr += tot_hdr;
    base_wire += tot_wire;
  }
  if (tid == 0) {
    uint64_t overflow = (bad || base_sl > R->cap || base_hdr > R->hdr_cap) ? 1 : 0;
    if (!bad && R->check_shape && (base_sl != R->want_slices || base_wire != R->want_wire)) overflow = 2;
    R->res[H2R_KEPT] = kept;
    R->res[H2R_DROPPED_STATUS] = n_status;
    R->res[H2R_UNROUTED] = n_unrouted;
    R->res[H2R_SLICES] = base_sl;
    R->res[H2R_HDR_BYTES] = base_hdr;
    R->res[H2R_WIRE_BYTES] = base_wire;
    R->res[H2R_OVERFLOW] = overflow;
  }
