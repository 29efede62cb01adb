// The body of a framing workgroup over ONE message table, for tables of up to H2_FRAME_ONE_MAX messages: included by
// k_h2_frame_one (the grid is the table's: H2_FRAME_GROUP = the block index) and by k_h2_frame_links (a link's share
// of the grid: the block index less the link's first workgroup), csrc/grdma_h2_kernels.h.  It expects msgs, nmsgs,
// max_frame, out, cap, hdr, hdr_cap and res in scope, as k_h2_frame_one's parameters are.
// (Source text rather than a device function: a function is simplified on its own before it is inlined, with
// generic pointers and without the kernel's launch bounds, and k_h2_frame_one then comes out with the operands of its
// 64-bit sums the other way round -- the same kernel, but not the same bytes as before it was shared  Tried and
// found to change it: a __forceinline__ function with the group as a parameter, a template over <bool SHARE> that reads
// blockIdx.x itself, the same as a plain inline function.  tools/h2_isa_compare.py is the comparison.)
  __shared__ uint64_t s_part[H2_EMIT_THREADS / 64][3];
  __shared__ uint64_t s_mine[H2_EMIT_THREADS / 64][3];
  __shared__ uint32_t s_mode[H2_EMIT_THREADS / 64];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = threadIdx.x >> 6;
  constexpr uint32_t PER = H2_EMIT_THREADS / 64;
  const uint64_t i0 = (uint64_t)H2_FRAME_GROUP * PER;
  // sizes of the messages in front of this workgroup's, one per thread per pass
  uint64_t a_sl = 0, a_hdr = 0, a_wire = 0;
  for (uint64_t j = threadIdx.x; j < i0; j += H2_EMIT_THREADS) {
    uint64_t n_sl, n_hdr, n_wire;
    uint32_t mode;
    h2_msg_size(msgs, j, max_frame, &n_sl, &n_hdr, &n_wire, &mode);
    a_sl += n_sl;
    a_hdr += n_hdr;
    a_wire += n_wire;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    a_sl += __shfl_xor(a_sl, d, 64);
    a_hdr += __shfl_xor(a_hdr, d, 64);
    a_wire += __shfl_xor(a_wire, d, 64);
  }
  if (lane == 0) {
    s_part[wave][0] = a_sl;
    s_part[wave][1] = a_hdr;
    s_part[wave][2] = a_wire;
    // ... and of my own message
    uint64_t n_sl = 0, n_hdr = 0, n_wire = 0;
    uint32_t mode = 0;
    if (i0 + wave < nmsgs) h2_msg_size(msgs, i0 + wave, max_frame, &n_sl, &n_hdr, &n_wire, &mode);
    s_mine[wave][0] = n_sl;
    s_mine[wave][1] = n_hdr;
    s_mine[wave][2] = n_wire;
    s_mode[wave] = mode;
  }
  __syncthreads();
  uint64_t b_sl = 0, b_hdr = 0, b_wire = 0;
  for (uint32_t w = 0; w < PER; w++) {
    b_sl += s_part[w][0];
    b_hdr += s_part[w][1];
    b_wire += s_part[w][2];
  }
  for (uint32_t w = 0; w < wave; w++) {
    b_sl += s_mine[w][0];
    b_hdr += s_mine[w][1];
    b_wire += s_mine[w][2];
  }
  const uint64_t i = i0 + wave;
  if (i + 1 == nmsgs && lane == 0) {  // the last message's wave knows the totals
    const uint64_t t_sl = b_sl + s_mine[wave][0], t_hdr = b_hdr + s_mine[wave][1];
    res->nslices = t_sl;
    res->hdr_bytes = t_hdr;
    res->wire_bytes = b_wire + s_mine[wave][2];
    res->overflow = (t_sl > cap || t_hdr > hdr_cap) ? 1 : 0;
  }
  if (i >= nmsgs) return;  // (wave-uniform)
  grdma_h2_msg_pos q;
  q.sl = b_sl;
  q.hdr = b_hdr;
  q.mode = s_mode[wave];
  q.pad = 0;
  h2_emit_message(msgs, i, nmsgs, max_frame, out, cap, hdr, hdr_cap, q, lane);
