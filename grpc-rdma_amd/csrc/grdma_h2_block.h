// The layout of the batch block: the one device block per process that holds a batch call of the HTTP/2 host side
// (csrc/grdma_h2_host_calls.inc: h2_batch_reserve).  Plain C++17 without HIP, so that the offset arithmetic is checked on
// the host alone (tests/cc/h2_block_host.cc); the callers pass the sizes of the device structs as numbers.
#pragma once
#include <cstdint>

// Parts are appended in order; each starts at the next multiple of its alignment (a power of two) behind the one before.
struct h2_block {
  uint64_t end = 0;  // behind the last part
  uint64_t add(uint64_t bytes, uint64_t align = 16) {
    const uint64_t at = (end + align - 1) & ~(align - 1);
    end = at + bytes;
    return at;
  }
  // what the call reserves: the parts and 16 bytes of slack behind the last one
  uint64_t total() const { return end + 16; }
};

// grdma_h2_deframe_batch and grdma_h2_deframe_messages_batch:
//   [deframe table | assembler table | call blocks | slice lists | zeroed results | event segments]
// [0, events) goes up in one copy, [results, ...) comes down in one copy.  Without assembly the two parts of the assembler
// have size 0 (asm_link = asm_call = 0) and the slice lists follow the deframe table.
struct h2_deframe_sizes {
  uint64_t link, slice, result, event;  // grdma_h2_link_deframe, grdma_slice_out, grdma_h2_deframe_result, grdma_h2_event
  uint64_t asm_link, asm_call;          // h2a_link, h2a_call
};
struct h2_deframe_block { uint64_t tab, asm_tab, asm_calls, slices, results, events, total; };
inline h2_deframe_block h2_deframe_block_layout(const h2_deframe_sizes& s, uint64_t n_items, uint64_t n_slices, uint64_t n_events) {
  h2_block b;  // (a braced list is evaluated left to right: the parts are appended in this order)
  return {b.add(s.link * n_items), b.add(s.asm_link * n_items), b.add(s.asm_call * n_items), b.add(s.slice * n_slices),
          b.add(s.result * n_items), b.add(s.event * n_events), b.total()};
}

// grdma_h2_fc_account_batch: [table | one call block per item]; all of it goes up.  (Targets and result blocks are
// words of the ledgers' own device blocks: nothing of them lies here.)
struct h2_fc_block { uint64_t tab, calls, end, total; };
inline h2_fc_block h2_fc_block_layout(uint64_t link, uint64_t call, uint64_t n_items) {
  h2_block b;
  return {b.add(link * n_items), b.add(call * n_items), b.end, b.total()};
}

// grdma_h2_hpenc_encode_batch: [table | one call block per item | nine result words per item]; [0, results) goes up in
// one copy, the result words come down in one copy.  (Nothing of a call lies in the encoders' own device blocks.)
struct h2_hpenc_block { uint64_t tab, calls, results, total; };
inline h2_hpenc_block h2_hpenc_block_layout(uint64_t link, uint64_t call, uint64_t n_items) {
  h2_block b;
  return {b.add(link * n_items), b.add(call * n_items), b.add(9 * sizeof(uint64_t) * n_items), b.total()};
}

// grdma_h2_meta_read_batch: [table | one h2m_call per item | link_grid h2m_wg per item, bad = ~0 | eight result words
// per item]; [0, results) goes up in one copy, the result words -- the emit launch writes all eight of every item --
// come down in one copy.  (The reader's own device block holds the constants and the counters only.)
struct h2_meta_block { uint64_t tab, calls, wgs, results, total; };
inline h2_meta_block h2_meta_block_layout(uint64_t link, uint64_t call, uint64_t wg, uint64_t link_grid, uint64_t n_items) {
  h2_block b;
  return {b.add(link * n_items), b.add(call * n_items), b.add(wg * link_grid * n_items), b.add(8 * sizeof(uint64_t) * n_items), b.total()};
}

// grdma_h2_calls_step_batch: [table | one h2c_call per item | eight result words per item]; [0, results) goes up in one
// copy, the result words -- the finish launch writes all eight of every item -- come down in one copy.  (Nothing of a
// step lies in the tables' own device blocks but their state and counters.)
struct h2_calls_block { uint64_t tab, calls, results, total; };
inline h2_calls_block h2_calls_block_layout(uint64_t link, uint64_t call, uint64_t n_items) {
  h2_block b;
  return {b.add(link * n_items), b.add(call * n_items), b.add(8 * sizeof(uint64_t) * n_items), b.total()};
}

// grdma_h2_reply_frame_batch: [table | one h2r_dev per item]; all of it goes up, the h2r_dev blocks come down.
struct h2_reply_block { uint64_t tab, devs, end, total; };
inline h2_reply_block h2_reply_block_layout(uint64_t link, uint64_t dev, uint64_t n_items) {
  h2_block b;
  return {b.add(link * n_items), b.add(dev * n_items), b.end, b.total()};
}
