// Receive flow control on the device (grdma_h2_fc): the window ledger of one transport.  The deframer's events of one
// call -> the received DATA bytes counted against the windows our SETTINGS announced, and the WINDOW_UPDATE frames that
// give them back (frame_window_update.cc: 13 bytes, length 4, type 8, flags 0, stream id, 31-bit increment), as a
// slice list of inlined slices the way grdma_h2_frame_messages writes one.  RFC 7540 6.9 with the position of the
// reference's RecvData (a frame counts where init_data_frame_parser sees its header); NOT a port of flow_control.cc:
// no BDP estimate, a fixed policy (docs/h2_deframer.md, "Receive flow control: the window ledger").
//
// Five launches of fixed shape behind the deframing; the event count is read on the device.  The keyed part (sums and
// first indices per stream) goes through a scratch table keyed by stream id -- open addressing from (id >> 1) & mask,
// as many slots as the parser's stream map, keys claimed with a compare-and-swap, values with vector atomics (add,
// min).  Kernel boundaries are the only agent-scope hand-over; inside the one-workgroup kernel barriers only.
//   k_h2_fc_clear    the scratch table, the mark words of the call's events, the call's accumulators
//   k_h2_fc_keys     per event: DATA frames add their size to the connection's sum (one atomic per wave) and, with
//                    status 0 on a stream the parser's map holds behind the call, claim the stream's slot (DATA on
//                    ids the transport never knew claims nothing: a peer cannot fill the table that way);
//                    STREAM_OPEN / STREAM_CLOSED claim it and leave their first event index there (min)
//   k_h2_fc_sums     per DATA frame with status 0: delivered to the stream's data parser when it lies in front of the
//                    stream's first STREAM_CLOSED and, for a stream opened in the call, behind its STREAM_OPEN -> the
//                    stream's sum (add) and the index of its first counted frame (min)
//   k_h2_fc_finish   one workgroup.  Per slot: a stream that neither opened nor closed in the call was delivered to
//                    only if the parser's map holds it open for reads (the deframer skips unknown and read-closed
//                    streams with status 0 too); violations; which streams get a frame.  Their first indices are
//                    marked in a bit per event, block scans over the words' popcounts give every stream its position
//                    (the order of the first counted frame); the connection's window, the caps, the result block
//   k_h2_fc_emit     fixed grid, one thread per 23-byte slice: the concatenated frames cut as grpc_slice_buffer_add
//                    merges inlined slices; writes nothing when the plan reported an overflow
#ifndef GRDMA_H2_FC_H
#define GRDMA_H2_FC_H
#include "grdma_h2_kernels.h"

#define H2FC_THREADS 256
#define H2FC_ONE_THREADS 512
#ifdef GRDMA_WAVE_EMU
#define H2FC_GRID 2  // (the emulator runs workgroups one after another: the kernels are grid-stride)
#else
#define H2FC_GRID 256
#endif
#define H2FC_NONE 0xffffffffu
#define H2FC_MAX_INC 0x7fffffffull  // the increment is 31 bits: a larger credit is cut to it (the rest stays pending)
#define H2FC_FRAME 13ull

enum { H2FC_FRAMES = 0, H2FC_SLICES = 1, H2FC_WIRE = 2, H2FC_CONN_BYTES = 3, H2FC_STREAM_BYTES = 4, H2FC_VIOLATIONS = 5,
       H2FC_FIRST_VIOLATOR = 6, H2FC_OVERFLOW = 7 };
enum { H2FC_V_CONN = 1, H2FC_V_STREAM = 2, H2FC_V_LOST = 4 };  // GRDMA_H2_FC_* of include/grdma_amd.h

// one stream of the call
struct h2fc_slot {
  uint32_t key;     // stream id, 0 = empty
  uint32_t first;   // event index of its first counted DATA frame
  uint32_t closed;  // ... of its first STREAM_CLOSED
  uint32_t opened;  // ... of its STREAM_OPEN
  unsigned long long sum;
  uint32_t emit, pad;
};
struct h2fc_upd {
  uint32_t stream, inc;
};
// one call: where the deframer left its output
struct h2fc_call {
  const grdma_h2_event* ev;
  const grdma_h2_deframe_result* res;
  uint64_t ev_cap;
};
// the ledger, resident in HBM
struct h2fc_dev {
  const grdma_h2_parser_dev* gp;
  uint64_t stream_window, conn_window, conn_threshold, max_updates;
  uint32_t tab_mask, pad0;
  h2fc_slot* tab;
  h2fc_upd* upd;       // max_updates frames
  // scratch sized by the events of a call
  uint64_t scratch_ev;
  uint32_t* mark;      // one bit per event: the first counted frame of a stream that gets a frame
  uint32_t* mark_pre;  // per word: the marks in front of it
  // where a call writes (a standalone call sets it; a pipe's are its own tables)
  grdma_sge* out;
  uint64_t cap;
  uint8_t* hdr;
  uint64_t hdr_cap;
  // state and counters since creation
  int64_t announced;
  uint64_t lost;
  uint64_t st_calls, st_conn_bytes, st_stream_bytes, st_frames, st_conn_over, st_stream_over;
  // the call's accumulators
  unsigned long long c_conn;
  uint32_t c_full, c_pad;
  uint64_t res[8];
};

namespace {

// the events of the call a ledger can account: none when the list overflowed (k_h2_fc_finish reports it)
__device__ __forceinline__ uint64_t h2fc_events(const h2fc_dev* F, const h2fc_call* call) {
  if (call->res->overflow) return 0;
  uint64_t n = call->res->nevents;
  if (n > call->ev_cap) n = call->ev_cap;
  return n > F->scratch_ev ? 0 : n;
}
__device__ __forceinline__ bool h2fc_lost(const h2fc_dev* F, const h2fc_call* call) {
  return call->res->overflow || call->res->nevents > F->scratch_ev || F->c_full;
}

// the slot of stream id, claimed if it has none (H2FC_NONE: the table is full)
__device__ __forceinline__ uint32_t h2fc_claim(h2fc_dev* F, uint32_t id) {
  const uint32_t m = F->tab_mask;
  uint32_t s = (id >> 1) & m;
  for (uint32_t probe = 0; probe <= m; probe++, s = (s + 1) & m) {
    uint32_t k = __hip_atomic_load(&F->tab[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0 && __hip_atomic_compare_exchange_strong(&F->tab[s].key, &k, id, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT))
      return s;
    if (k == id) return s;  // (a failed exchange leaves the winner's key in k)
  }
  atomicExch(&F->c_full, 1u);
  return H2FC_NONE;
}
__device__ __forceinline__ uint32_t h2fc_find(const h2fc_dev* F, uint32_t id) {
  const uint32_t m = F->tab_mask;
  uint32_t s = (id >> 1) & m;
  for (uint32_t probe = 0; probe <= m; probe++, s = (s + 1) & m) {
    const uint32_t k = F->tab[s].key;
    if (k == id) return s;
    if (k == 0) return H2FC_NONE;
  }
  return H2FC_NONE;
}

__device__ __forceinline__ bool h2fc_is_data(const grdma_h2_event& e) { return e.kind == EV_FRAME && e.a == 0; }

__global__ __launch_bounds__(H2FC_THREADS) void k_h2_fc_clear(h2fc_dev* F, const h2fc_call* call) {
  const uint64_t t0 = (uint64_t)blockIdx.x * H2FC_THREADS + threadIdx.x, step = (uint64_t)gridDim.x * H2FC_THREADS;
  const h2fc_slot empty = {0, H2FC_NONE, H2FC_NONE, H2FC_NONE, 0, 0, 0};
  for (uint64_t s = t0; s <= F->tab_mask; s += step) F->tab[s] = empty;
  uint64_t n = call->res->overflow ? 0 : call->res->nevents;
  if (n > F->scratch_ev) n = 0;
  const uint64_t words = (n + 31) / 32;
  for (uint64_t w = t0; w < words; w += step) F->mark[w] = 0;
  if (t0 == 0) {
    F->c_conn = 0;
    F->c_full = 0;
  }
}

__global__ __launch_bounds__(H2FC_THREADS) void k_h2_fc_keys(h2fc_dev* F, const h2fc_call* call) {
  const uint64_t n = h2fc_events(F, call);
  const int lane = threadIdx.x & 63;
  uint64_t mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * H2FC_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * H2FC_THREADS) {
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
}

__global__ __launch_bounds__(H2FC_THREADS) void k_h2_fc_sums(h2fc_dev* F, const h2fc_call* call) {
  if (h2fc_lost(F, call)) return;
  const uint64_t n = h2fc_events(F, call);
  for (uint64_t i = (uint64_t)blockIdx.x * H2FC_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * H2FC_THREADS) {
    const grdma_h2_event e = call->ev[i];
    if (!h2fc_is_data(e) || (e.b >> 8) != 0 || e.c == 0) continue;
    const uint32_t s = h2fc_find(F, e.c);
    if (s == H2FC_NONE) continue;
    const uint32_t closed = F->tab[s].closed, opened = F->tab[s].opened;
    if ((uint32_t)i > closed || (opened != H2FC_NONE && (uint32_t)i < opened)) continue;
    atomicAdd(&F->tab[s].sum, (unsigned long long)e.d);
    atomicMin(&F->tab[s].first, (uint32_t)i);
  }
}

__global__ __launch_bounds__(H2FC_ONE_THREADS) void k_h2_fc_finish(h2fc_dev* F, const h2fc_call* call) {
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
}

// byte o of a frame: 24-bit length 4, type 8, flags 0, the stream id, the increment (big-endian)
__device__ __forceinline__ uint32_t h2fc_byte(uint32_t stream, uint32_t inc, uint32_t o) {
  if (o < 5) return o == 2 ? 4u : o == 3 ? 8u : 0u;
  if (o < 9) return ((stream & 0x7fffffffu) >> (8 * (8 - o))) & 0xffu;
  return ((inc & 0x7fffffffu) >> (8 * (12 - o))) & 0xffu;
}

// bytes [b0, b0 + 8) of a slice that starts r0 bytes into frame 0 of the three frames it may touch (the values travel
// as scalars: a frame picked from an array by a run-time index would live in scratch memory)
__device__ __forceinline__ uint64_t h2fc_word(uint32_t r0, uint32_t b0, uint32_t len, uint32_t s0, uint32_t i0, uint32_t s1,
                                              uint32_t i1, uint32_t s2, uint32_t i2) {
  uint64_t q = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint32_t b = b0 + j, t = r0 + b;
    const uint32_t df = t >= 26u ? 2u : t >= 13u ? 1u : 0u, o = t - 13u * df;
    const uint32_t st = df == 0 ? s0 : df == 1 ? s1 : s2, in = df == 0 ? i0 : df == 1 ? i1 : i2;
    const uint64_t v = b < len ? h2fc_byte(st, in, o) : 0u;
    q |= v << (8 * j);
  }
  return q;
}

__global__ __launch_bounds__(H2FC_THREADS) void k_h2_fc_emit(const h2fc_dev* F) {
  if (F->res[H2FC_OVERFLOW]) return;  // (nothing half-written; a lost call has no slices)
  const uint64_t frames = F->res[H2FC_FRAMES], slices = F->res[H2FC_SLICES], wire = F->res[H2FC_WIRE];
  for (uint64_t k = (uint64_t)blockIdx.x * H2FC_THREADS + threadIdx.x; k < slices; k += (uint64_t)gridDim.x * H2FC_THREADS) {
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
}

}  // namespace
#endif  // GRDMA_H2_FC_H
