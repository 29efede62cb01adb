// Send flow control on the device (grdma_h2_sw, "send windows"): the peer's windows of one transport, kept in HBM, fed
// from the deframer's events (the peer's WINDOW_UPDATE and SETTINGS frames arrive on the parser of the same transport),
// and a framer that never sends a byte the peer has not allowed.  The sending rule is the reference's
// DataSendContext::max_outgoing (writing.cc): min(peer MAX_FRAME_SIZE, stream remote window, transport remote window),
// the stream's window being peer INITIAL_WINDOW_SIZE + delta.  A fixed policy, NOT a port of flow_control.cc
// (docs/h2_deframer.md, "Send flow control: the peer's windows"; the rules: include/grdma_amd.h).
//
// State: the connection's window (int64, may go negative), the peer's INITIAL_WINDOW_SIZE and MAX_FRAME_SIZE, per stream
// a signed delta (credit received - bytes sent) in a table keyed by stream id -- open addressing from (id >> 1) & mask, as
// many slots as the parser's map, keys claimed with a compare-and-swap (as h2fc_claim), a missing entry = delta 0 -- and
// the carry: the control frame whose payload the end of the previous call cut.
//
// Intake, three launches of fixed shape behind a deframing (the event count is read on the device):
//   k_h2_sw_clear    the second table, the call's accumulators, the outgoing carry
//   k_h2_sw_take     the entries whose stream the parser's map still holds move to the second table (claim + add: a
//                    stream that left the map leaves the table, so it never fills with dead entries); then one thread
//                    per WINDOW_UPDATE / SETTINGS frame event walks the frame's PAYLOAD events (bounded by the event
//                    count), reads the bytes from the receive arena and, at the frame's last byte, adds the increment
//                    to the connection's sum or its stream's credit (vector atomics) or hands in the frame's settings
//                    (a 64-bit max of event index << 32 | value: the last frame wins).  The grid's first thread continues
//                    the carried frame over the PAYLOAD events in front of the first FRAME event.  ONE lane walks one
//                    SETTINGS frame byte by byte: they are rare and six entries long in practice.
//   k_h2_sw_finish   one workgroup: per slot the credit goes into the delta (clamped so that the window stays within
//                    2^31 - 1), the connection, the settings, the carry, the result block; the tables change roles
// Framing, two launches as k_h2_reply_plan / k_h2_reply_emit:
//   k_h2_sw_plan     one workgroup, at most H2_FRAME_ONE_MAX messages in blocks of its size.  The grant in two prefix
//                    sums: a keyed exclusive scan of the remaining bytes per stream (per wave tile one pass per distinct
//                    stream, as k_h2_asm_tiles: ONE lane looks the stream up and claims its slot, a masked scan sums;
//                    across the tiles of a block through lists of the tiles' sums in LDS, across blocks through the
//                    stream's slot) against the stream's window, then a block scan of the result against the
//                    connection's.  The granted pieces are compacted and laid out as k_h2_frame_index lays messages out
//                    (closed form, or sequentially around pieces that leave an inlined slice at the back); the caps;
//                    only then the windows move.
//   k_h2_sw_emit     fixed grid, one wave per piece by static grid-stride; writes nothing after an overflow
// Kernel boundaries are the only agent-scope hand-over; inside the one-workgroup kernels barriers only.
// The same five stages over a table of links (k_h2_links_sw_*: the send windows of many transports in the same three and
// two launches) stand at the end of the file; both families include their bodies from csrc/grdma_h2_sw_stage.inc.
#ifndef GRDMA_H2_SW_H
#define GRDMA_H2_SW_H
#include "grdma_h2_kernels.h"

#define H2SW_THREADS 256
#define H2SW_PLAN_THREADS 512
#ifdef GRDMA_WAVE_EMU
#define H2SW_GRID 2  // (the emulator runs workgroups one after another: the kernels are grid-stride)
#else
#define H2SW_GRID 256
#endif
#define H2SW_NONE 0xffffffffu
#define H2SW_MAXW 0x7fffffffll

enum { H2SW_I_UPDATES = 0, H2SW_I_CONN = 1, H2SW_I_STREAMS = 2, H2SW_I_SETTINGS = 3, H2SW_I_VIOLATIONS = 4, H2SW_I_FIRST = 5,
       H2SW_I_LIVE = 6, H2SW_I_OVERFLOW = 7 };
enum { H2SW_F_DONE = 0, H2SW_F_HELD = 1, H2SW_F_SLICES = 2, H2SW_F_HDR = 3, H2SW_F_WIRE = 4, H2SW_F_GRANTED = 5, H2SW_F_STALL = 6,
       H2SW_F_OVERFLOW = 7 };
enum { H2SW_V_INCREMENT = 1, H2SW_V_WINDOW = 2, H2SW_V_SETTINGS = 4, H2SW_V_LOST = 8 };  // GRDMA_H2_SW_* of include/grdma_amd.h
enum { H2SW_STALL_CONN = 1, H2SW_STALL_STREAM = 2, H2SW_STALL_UNKNOWN = 4 };

// one stream's entry
struct h2sw_slot {
  uint32_t key;    // stream id, 0 = empty
  uint32_t first;  // intake: event position of the stream's first WINDOW_UPDATE of the call
  long long delta; // credit received - bytes sent
  unsigned long long credit;  // intake: the call's sum of increments
  unsigned long long run;     // framing: the remaining bytes of the call's messages so far (the keyed scan's carry)
  unsigned long long sent;    // framing: the bytes the call grants
};
// a control frame in flight: what a thread holds while it walks a frame, and what a call's end leaves behind
struct h2sw_frame {
  uint32_t type;    // 8 WINDOW_UPDATE, 4 SETTINGS, 0 none
  uint32_t stream;
  uint32_t nbytes;  // bytes of the increment / of the current settings entry taken in
  uint32_t have;    // SETTINGS: 1 = iws, 2 = mfs hold a value of this frame
  uint64_t acc;     // those bytes, big-endian
  uint32_t iws, mfs;
};
// one call: where the deframer left its output and what it read
struct h2sw_call {
  const grdma_h2_event* ev;
  const grdma_h2_deframe_result* res;
  const grdma_slice_out* sl;
  const uint8_t* arena;
  uint64_t ev_cap, nsl;
  uint64_t skipped;  // a standalone deframing in front of this one was never taken in
};
// one granted piece: bytes [p, p + g) of [5-byte header | payload]
struct h2sw_piece {
  const uint8_t* payload;
  uint64_t len;
  uint32_t stream_id, flags;
  uint64_t p, g;
};
// the send windows, resident in HBM
struct h2sw_dev {
  const grdma_h2_parser_dev* gp;
  h2sw_slot* tabs[2];
  h2sw_piece* pieces;  // H2_FRAME_ONE_MAX
  grdma_h2_msg_pos* pos;
  uint64_t* prog_out;
  uint32_t* slot_of;   // per message of a framing call: its stream's slot
  uint32_t tab_mask, pad0;
  // a framing call (the host sets it)
  const grdma_h2_msg_dev* msgs;
  const uint64_t* prog_in;
  uint64_t nmsgs;
  uint64_t max_frame;
  grdma_sge* out;
  uint64_t cap;
  uint8_t* hdr;
  uint64_t hdr_cap;
  // state and counters since creation (the device's)
  long long conn;
  uint32_t iws, pmf;
  uint32_t cur, lost;
  h2sw_frame carry, carry_out;
  uint64_t st_intakes, st_updates, st_settings, st_violations, st_frame_calls, st_sent;
  // an intake's accumulators
  unsigned long long c_conn, c_first, c_iws, c_mfs;
  uint32_t c_applied, c_nset, c_bad_inc, c_bad_set, c_conn_first, c_full;
  uint64_t npieces;
  uint64_t res[8];   // H2SW_I_*
  uint64_t fres[8];  // H2SW_F_*
};

namespace {

// the slot of stream id in t, claimed if it has none (H2SW_NONE: the table is full)
__device__ __forceinline__ uint32_t h2sw_claim(h2sw_slot* t, uint32_t m, uint32_t id) {
  uint32_t s = (id >> 1) & m;
  for (uint32_t probe = 0; probe <= m; probe++, s = (s + 1) & m) {
    uint32_t k = __hip_atomic_load(&t[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0 && __hip_atomic_compare_exchange_strong(&t[s].key, &k, id, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT))
      return s;
    if (k == id) return s;  // (a failed exchange leaves the winner's key in k)
  }
  return H2SW_NONE;
}

// the call's events an intake can take in: none after an overflow or a connection error
__device__ __forceinline__ bool h2sw_lost(const h2sw_call* call) { return call->res->overflow || call->res->nevents > call->ev_cap; }
__device__ __forceinline__ bool h2sw_taken(const h2sw_call* call) { return !h2sw_lost(call) && call->res->error == 0; }

// an offence at event position v on stream id: the first one is reported
__device__ __forceinline__ void h2sw_offence(h2sw_dev* F, uint32_t v, uint32_t id) {
  atomicMin(&F->c_first, ((unsigned long long)v << 32) | id);
}

// one more payload byte of the frame f (which began at event position v)
__device__ __forceinline__ void h2sw_byte(h2sw_dev* F, h2sw_frame& f, uint32_t byte, uint32_t v) {
  f.acc = (f.acc << 8) | byte;
  f.nbytes++;
  if (f.type != FT_SETTINGS || f.nbytes < 6) return;
  const uint32_t id = (uint32_t)(f.acc >> 32) & 0xffffu, val = (uint32_t)f.acc;
  f.acc = 0;
  f.nbytes = 0;
  if (id == 4) {  // INITIAL_WINDOW_SIZE
    if (val > (uint32_t)H2SW_MAXW) {
      atomicAdd(&F->c_bad_set, 1u);
      h2sw_offence(F, v, 0);
    } else {
      f.iws = val;
      f.have |= 1u;
    }
  } else if (id == 5) {  // MAX_FRAME_SIZE
    if (val < 16384u || val > 16777215u) {
      atomicAdd(&F->c_bad_set, 1u);
      h2sw_offence(F, v, 0);
    } else {
      f.mfs = val;
      f.have |= 2u;
    }
  }
}

// the frame f has its last byte: its effect goes to the call's accumulators and the second table neu
__device__ __forceinline__ void h2sw_complete(h2sw_dev* F, h2sw_slot* neu, const h2sw_frame& f, uint32_t v) {
  if (f.type == FT_WINDOW_UPDATE) {
    const uint32_t inc = (uint32_t)f.acc;
    if (f.nbytes != 4) return;  // (the deframer has checked the length: cannot be)
    if (inc == 0 || (inc >> 31)) {
      atomicAdd(&F->c_bad_inc, 1u);
      h2sw_offence(F, v, f.stream);
    } else if (f.stream == 0) {
      atomicAdd(&F->c_conn, (unsigned long long)inc);
      atomicMin(&F->c_conn_first, v);
      atomicAdd(&F->c_applied, 1u);
    } else if (tab_find(F->gp->tab, F->gp->tab_mask, f.stream) >= 0) {  // (the map behind the call)
      const uint32_t s = h2sw_claim(neu, F->tab_mask, f.stream);
      if (s == H2SW_NONE) {
        atomicExch(&F->c_full, 1u);
      } else {
        atomicAdd(&neu[s].credit, (unsigned long long)inc);
        atomicMin(&neu[s].first, v);
        atomicAdd(&F->c_applied, 1u);
      }
    }
  } else {
    // the values take effect with the frame's last byte; of several frames the last wins
    if (f.have & 1u) atomicMax(&F->c_iws, ((unsigned long long)(v + 1u) << 32) | f.iws);
    if (f.have & 2u) atomicMax(&F->c_mfs, ((unsigned long long)(v + 1u) << 32) | f.mfs);
    atomicAdd(&F->c_nset, 1u);
  }
}

// The frame f, which began at event position v, over the PAYLOAD events from j on: every walk is bounded by the event
// count.  A frame the call's end cuts becomes the outgoing carry (at most one frame of a call is open at its end).
__device__ __forceinline__ void h2sw_walk(h2sw_dev* F, const h2sw_call* call, h2sw_slot* neu, h2sw_frame f, uint64_t j, uint64_t n,
                                          uint32_t v) {
  for (; j < n; j++) {
    const grdma_h2_event pe = call->ev[j];
    if (pe.kind != EV_PAYLOAD) return;  // (a payload run ends with its is_last event: cannot be)
    if (pe.slice < call->nsl) {
      const grdma_slice_out sl = call->sl[pe.slice];
      if ((uint64_t)pe.a + pe.b <= sl.len) {
        const uint8_t* src = call->arena + sl.off + pe.a;
        for (uint32_t k = 0; k < pe.b; k++) h2sw_byte(F, f, src[k], v);
      }
    }
    if (pe.c) {
      h2sw_complete(F, neu, f, v);
      return;
    }
  }
  F->carry_out = f;
}

// The stages' bodies are source text (csrc/grdma_h2_sw_stage.inc); the k_h2_links_sw_* kernels at the end of this file
// include the same text over a table of links.
#define H2SW_BLK blockIdx.x
#define H2SW_NBLK gridDim.x
__global__ __launch_bounds__(H2SW_THREADS) void k_h2_sw_clear(h2sw_dev* F) {
#define H2SW_STAGE 1
#include "grdma_h2_sw_stage.inc"
#undef H2SW_STAGE
}

__global__ __launch_bounds__(H2SW_THREADS) void k_h2_sw_take(h2sw_dev* F, const h2sw_call* call) {
#define H2SW_STAGE 2
#include "grdma_h2_sw_stage.inc"
#undef H2SW_STAGE
}

__global__ __launch_bounds__(H2SW_THREADS) void k_h2_sw_finish(h2sw_dev* F, const h2sw_call* call) {
#define H2SW_STAGE 3
#include "grdma_h2_sw_stage.inc"
#undef H2SW_STAGE
}
#undef H2SW_BLK
#undef H2SW_NBLK

// ---------------------------------------------------------------------------------------------------- the framer
// The layout of a piece is the layout of a message (walk_message, h2_emit_message) started at an offset and ended by the
// grant.  A piece that ends within the 5-byte header (p + g <= 5: a window cut there, or an empty message) leaves an
// inlined slice at the back of the outbuf, into which the next frame header merges.
__device__ __forceinline__ bool h2sw_tail_inlined(const h2sw_piece& q) { return q.p + q.g <= 5; }

// closed form: the piece starts behind a by-reference slice, at the message's start with more than its header granted
// or inside its payload -- every frame is [inlined frame header (+ message header) | payload piece]
__device__ __forceinline__ bool h2sw_plain(const h2sw_piece* pc, uint64_t k, uint32_t mf) {
  const h2sw_piece q = pc[k];
  return mf > 5 && (q.p >= 5 || (q.p == 0 && q.g >= 6)) && (k == 0 || !h2sw_tail_inlined(pc[k - 1]));
}

// sequential layout of ONE piece given the state of the outbuf's back slice: walk_message from byte p, g bytes long
template <bool EMIT>
__device__ void h2sw_walk_piece(const h2sw_piece& m, uint32_t max_frame, frame_walk* w, grdma_sge* out, uint8_t* hdr, uint64_t cap,
                                uint64_t hdr_cap, uint64_t* overflow) {
  const uint64_t h5 = (uint64_t)((m.flags & 1) ? 1 : 0) | ((m.len >> 24) & 0xFF) << 8 | ((m.len >> 16) & 0xFF) << 16 |
                      ((m.len >> 8) & 0xFF) << 24 | (m.len & 0xFF) << 32;
  uint64_t h5_left = m.p < 5 ? 5 - m.p : 0, pay_off = m.p > 5 ? m.p - 5 : 0;
  uint64_t fcb = 5 + m.len - m.p, left = m.g;
  while (left > 0) {
    const uint64_t send = left < max_frame ? left : max_frame;
    const bool whole = (fcb == send);  // grpc_slice_buffer_move_into: every slice via add()
    const bool last = (m.flags & 2) && whole;
    const uint64_t fh = ((send >> 16) & 0xFF) | ((send >> 8) & 0xFF) << 8 | (send & 0xFF) << 16 | (uint64_t)(last ? 1 : 0) << 32 |
                        (uint64_t)((m.stream_id >> 24) & 0xFF) << 40 | (uint64_t)((m.stream_id >> 16) & 0xFF) << 48 |
                        (uint64_t)((m.stream_id >> 8) & 0xFF) << 56;
    add_inlined<EMIT>(w, fh, (uint64_t)(m.stream_id & 0xFF), 9, true, out, hdr, cap, hdr_cap, overflow);
    uint64_t n = send;
    if (h5_left > 0) {
      const uint64_t take = n < h5_left ? n : h5_left;
      const bool merge = whole || n >= h5_left;  // n < slice length: split, the head goes in un-merged (add_indexed)
      add_inlined<EMIT>(w, h5 >> (8 * (5 - h5_left)), 0, (uint32_t)take, merge, out, hdr, cap, hdr_cap, overflow);
      h5_left -= take;
      n -= take;
    }
    if (n > 0) {
      add_ref<EMIT>(w, m.payload + pay_off, n, out, cap, overflow);
      pay_off += n;
    }
    fcb -= send;
    left -= send;
  }
}

// sizes of piece k and who lays it out (grdma_h2_msg_pos::mode)
__device__ __forceinline__ void h2sw_piece_size(const h2sw_piece* pc, uint64_t k, uint32_t mf, uint64_t* n_sl, uint64_t* n_hdr,
                                                uint64_t* n_wire, uint32_t* mode) {
  if (h2sw_plain(pc, k, mf)) {
    const uint64_t F = (pc[k].g + mf - 1) / mf;
    *n_sl = 2 * F;
    *n_hdr = 32 * F;
    *n_wire = 9 * F + pc[k].g;
    *mode = 1;
    return;
  }
  // incoming back-slice state: replay the run of pieces in front that hand an inlined slice on
  uint64_t overflow = 0;
  uint64_t j = k;
  while (j > 0 && h2sw_tail_inlined(pc[j - 1])) j--;
  frame_walk pre = {0, 0, 0, 0};
  for (; j < k; j++) h2sw_walk_piece<false>(pc[j], mf, &pre, nullptr, nullptr, ~0ull, ~0ull, &overflow);
  frame_walk me = {0, 0, 0, pre.back_inl};
  h2sw_walk_piece<false>(pc[k], mf, &me, nullptr, nullptr, ~0ull, ~0ull, &overflow);
  *n_sl = me.nslices;
  *n_hdr = me.hdr_off;
  *n_wire = me.wire;
  *mode = (k == 0 || !h2sw_tail_inlined(pc[k - 1])) ? 2u : 0u;
}

// one wave lays out piece k at position q
__device__ __forceinline__ void h2sw_emit_piece(const h2sw_piece* pc, uint64_t k, uint64_t npieces, uint32_t mf, grdma_sge* out,
                                                uint64_t cap, uint8_t* hdr, uint64_t hdr_cap, const grdma_h2_msg_pos q, int lane) {
  if (q.mode == 2) {
    if (lane == 0) {
      uint64_t overflow = 0;  // (the plan has reported it; here it only keeps the stores inside the arrays)
      frame_walk me = {q.sl, q.hdr, 0, 0};
      for (uint64_t j = k;;) {
        h2sw_walk_piece<true>(pc[j], mf, &me, out, hdr, cap, hdr_cap, &overflow);
        if (!h2sw_tail_inlined(pc[j]) || j + 1 >= npieces) break;
        j++;
      }
    }
    return;
  }
  if (q.mode != 1) return;
  const h2sw_piece m = pc[k];
  const uint64_t F = (m.g + mf - 1) / mf;
  for (uint64_t j = (uint64_t)lane; j < F; j += 64) {
    const uint64_t slot = q.sl + 2 * j, hoff = q.hdr + 32 * j;
    if (slot + 2 > cap || hoff + 32 > hdr_cap) break;  // (reported by the plan)
    const uint64_t done = j * mf, at = m.p + done;  // at: the frame's first byte in [header | payload]
    const uint64_t send = m.g - done < mf ? m.g - done : mf;
    const uint64_t last = ((m.flags & 2) && at + send == 5 + m.len) ? 1 : 0;
    uint64_t w0 = ((send >> 16) & 0xFF) | (((send >> 8) & 0xFF) << 8) | ((send & 0xFF) << 16) | (last << 32) |
                  ((uint64_t)((m.stream_id >> 24) & 0xFF) << 40) | ((uint64_t)((m.stream_id >> 16) & 0xFF) << 48) |
                  ((uint64_t)((m.stream_id >> 8) & 0xFF) << 56);
    uint64_t w1 = (uint64_t)(m.stream_id & 0xFF);
    uint64_t hl = 9;
    if (at == 0) {
      w1 |= (uint64_t)((m.flags & 1) ? 1 : 0) << 8 | ((m.len >> 24) & 0xFF) << 16 | ((m.len >> 16) & 0xFF) << 24 |
            ((m.len >> 8) & 0xFF) << 32 | (m.len & 0xFF) << 40;
      hl = 14;
    }
    uint8_t* hp = hdr + hoff;
    u64x2 hv;
    hv.x = w0;
    hv.y = w1;
    if (((uint64_t)hp & 15) == 0) {
      *reinterpret_cast<u64x2*>(hp) = hv;  // (the slot is 32 bytes: the bytes behind the header are nobody's)
    } else {
      for (uint64_t b = 0; b < hl; b++) hp[b] = (uint8_t)((b < 8 ? w0 >> (8 * b) : w1 >> (8 * (b - 8))) & 0xFF);
    }
    u64x2 e0, e1;
    e0.x = (uint64_t)hp;
    e0.y = hl;
    e1.x = (uint64_t)(m.payload + (at == 0 ? 0 : at - 5));
    e1.y = at == 0 ? send - 5 : send;
    *reinterpret_cast<u64x2*>(&out[slot]) = e0;
    *reinterpret_cast<u64x2*>(&out[slot + 1]) = e1;
  }
}

// exclusive scan of one value per thread over the plan's workgroup; returns the prefix and, in *total, the sum
__device__ __forceinline__ uint64_t h2sw_block_scan(uint64_t v, uint64_t* ws, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t incl = wave_incl_scan(v, lane);
  if (lane == 63) ws[wave] = incl;
  __syncthreads();
  uint64_t base = 0, tot = 0;
  for (int w = 0; w < H2SW_PLAN_THREADS / 64; w++) {
    const uint64_t sum = ws[w];
    if (w < wave) base += sum;
    tot += sum;
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

__global__ __launch_bounds__(H2SW_PLAN_THREADS) void k_h2_sw_plan(h2sw_dev* F) {
#define H2SW_STAGE 4
#include "grdma_h2_sw_stage.inc"
#undef H2SW_STAGE
}

__global__ __launch_bounds__(H2_EMIT_THREADS) void k_h2_sw_emit(const h2sw_dev* F) {
#define H2SW_STAGE 5
#include "grdma_h2_sw_stage.inc"
#undef H2SW_STAGE
}

// ---- the five kernels over a table of L <= H2SW_LINKS_MAX links (the send windows of a batch): three launches an
// intake and two a framing however many links.  Nothing is shared between the links -- every entry has its own h2sw_dev
// (tables, piece and position scratch, accumulators, result blocks) and its own call block -- so every atomic stays on
// the link's own h2sw_dev and tables, and a lost call, a connection error, a skipped deframing, a cap overflow or an empty
// event list stay with their link.  The entry is loaded with a uniform index: it sits in scalar registers, as the single
// kernels' parameters do.
//   clear, take   link l owns the workgroups [l * H2SW_LINK_GRID, (l + 1) * H2SW_LINK_GRID): the single kernel's
//                 grid-stride inside that share; the share's first thread clears the accumulators and continues the
//                 carried frame
//   finish, plan  grid L: workgroup l is the one workgroup of link l -- L finishes, L plans side by side
//   emit          a fixed grid; the pieces of ALL links by one static grid-stride, so a stalled or overflowed link idles
//                 nobody: every workgroup builds the exclusive prefix of the links' piece counts in LDS (one block scan,
//                 one link per thread; a link whose result block reports an overflow contributes 0 and gets nothing
//                 written), a wave finds the link of its piece by binary search over it (wave-uniform: the link's
//                 pointers stay scalar) and lays the piece out with that link's tables and frame size.  A piece's run of
//                 inlined slices (mode 2) ends with its link's last piece: npieces is the link's.
// The kernel boundary is the only agent-scope hand-over; inside the finish and the plan barriers only.
#define H2SW_LINKS_MAX 256  // (= GRDMA_H2_BATCH_MAX, include/grdma_amd.h; one thread per link in the emit's block scan)
#ifdef GRDMA_WAVE_EMU
#define H2SW_LINK_GRID 2
#else
#define H2SW_LINK_GRID 8    // 2048 threads per link: an event or a slot per thread up to 2048, grid-stride beyond
#endif
struct h2sw_link {
  h2sw_dev* F;
  const h2sw_call* call;  // (an intake's; a framing leaves it NULL)
};
static_assert(H2SW_LINKS_MAX <= H2_EMIT_THREADS, "k_h2_links_sw_emit scans one link per thread");
// The table is written by the host in front of the launch and only read on the device, so it is read as constant
// memory (as H2FC_ENTRY, csrc/grdma_h2_fc.h): pointers loaded from there are taken as global ones, and the link
// kernels address as their single twins do.
#ifdef GRDMA_WAVE_EMU
#define H2SW_ENTRY(tab, l) ((tab)[l])
#else
#define H2SW_ENTRY(tab, l) (((const __attribute__((address_space(4))) h2sw_link*)(tab))[l])
#endif

// (a link's share of the grid)
#define H2SW_BLK (blockIdx.x % H2SW_LINK_GRID)
#define H2SW_NBLK H2SW_LINK_GRID
__global__ __launch_bounds__(H2SW_THREADS) void k_h2_links_sw_clear(const h2sw_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2SW_LINK_GRID;
  if (l >= nlinks) return;
  h2sw_dev* const F = H2SW_ENTRY(tab, l).F;
#define H2SW_STAGE 1
#include "grdma_h2_sw_stage.inc"
#undef H2SW_STAGE
}

__global__ __launch_bounds__(H2SW_THREADS) void k_h2_links_sw_take(const h2sw_link* __restrict__ tab, uint32_t nlinks) {
  const uint32_t l = blockIdx.x / H2SW_LINK_GRID;
  if (l >= nlinks) return;
  h2sw_dev* const F = H2SW_ENTRY(tab, l).F;
  const h2sw_call* const call = H2SW_ENTRY(tab, l).call;
#define H2SW_STAGE 2
#include "grdma_h2_sw_stage.inc"
#undef H2SW_STAGE
}

__global__ __launch_bounds__(H2SW_THREADS) void k_h2_links_sw_finish(const h2sw_link* __restrict__ tab) {
  h2sw_dev* const F = H2SW_ENTRY(tab, blockIdx.x).F;
  const h2sw_call* const call = H2SW_ENTRY(tab, blockIdx.x).call;
#define H2SW_STAGE 3
#include "grdma_h2_sw_stage.inc"
#undef H2SW_STAGE
}
#undef H2SW_BLK
#undef H2SW_NBLK

__global__ __launch_bounds__(H2SW_PLAN_THREADS) void k_h2_links_sw_plan(const h2sw_link* __restrict__ tab) {
  h2sw_dev* const F = H2SW_ENTRY(tab, blockIdx.x).F;
#define H2SW_STAGE 4
#include "grdma_h2_sw_stage.inc"
#undef H2SW_STAGE
}

__global__ __launch_bounds__(H2_EMIT_THREADS) void k_h2_links_sw_emit(const h2sw_link* __restrict__ tab, uint32_t nlinks) {
  __shared__ uint64_t s_pre[H2SW_LINKS_MAX + 1];  // exclusive prefix of the links' pieces; [nlinks]: the total
  __shared__ uint64_t s_wave[H2_EMIT_THREADS / 64];
  const int lane = threadIdx.x & 63;
  const uint32_t wv = uni32(threadIdx.x >> 6);
  uint64_t mine = 0;
  if (threadIdx.x < nlinks) {
    const h2sw_dev* const F = tab[threadIdx.x].F;
    if (!F->fres[H2SW_F_OVERFLOW]) mine = F->npieces;  // (nothing half-written)
  }
  const uint64_t incl = wave_incl_scan(mine, lane);
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  uint64_t base = 0;
  for (uint32_t w = 0; w < wv; w++) base += s_wave[w];
  if (threadIdx.x == 0) s_pre[0] = 0;
  s_pre[threadIdx.x + 1] = base + incl;
  __syncthreads();
  const uint64_t total = s_pre[nlinks];
  const uint64_t waves = (uint64_t)gridDim.x * (H2_EMIT_THREADS / 64);
  for (uint64_t g = (uint64_t)blockIdx.x * (H2_EMIT_THREADS / 64) + wv; g < total; g += waves) {
    uint32_t ll = 0, lh = nlinks;  // the last link whose prefix <= g (a link without pieces shares its prefix with the next)
    while (lh - ll > 1) {
      const uint32_t mid = (ll + lh) / 2;
      if (uni64(s_pre[mid]) <= g) ll = mid;
      else lh = mid;
    }
    const h2sw_dev* const F = H2SW_ENTRY(tab, ll).F;
    const uint64_t k = g - uni64(s_pre[ll]);
    const uint32_t mf = (uint32_t)(F->max_frame < F->pmf ? F->max_frame : F->pmf);
    h2sw_emit_piece(F->pieces, k, F->npieces, mf, F->out, F->cap, F->hdr, F->hdr_cap, F->pos[k], lane);
  }
}

}  // namespace
#endif  // GRDMA_H2_SW_H
