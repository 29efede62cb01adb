// The layout of the HTTP/2 batch block (grpc-rdma_amd/csrc/grdma_h2_block.h) on the host: the three layouts of the batch
// calls for 1, 2 and GRDMA_H2_BATCH_MAX items -- items without slices and without event capacity, odd slice counts, struct
// sizes that are no multiples of 16 -- against the offset arithmetic the batch calls carried themselves before the
// builder, written out again below.  Every part is then written end to end into a heap buffer of exactly `total` bytes:
// built with -fsanitize=address,undefined (tests/test_h2_block_host.py) an overrun ends the program.
#include <cstdio>
#include <cstring>
#include <vector>

#include "grdma_h2_block.h"

static const uint64_t BATCH_MAX = 256;  // GRDMA_H2_BATCH_MAX (include/grdma_amd.h)
static int g_failed = 0;

#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      printf("FAIL %s: ", #cond);       \
      printf(__VA_ARGS__);              \
      printf("\n");                     \
      g_failed++;                       \
    }                                   \
  } while (0)

static uint64_t up16(uint64_t v) { return (v + 15) & ~15ull; }

struct part { uint64_t off, bytes; };

// aligned, in order, no overlap, inside total; then every byte of every part and of the slack written, and every part
// still there at the end
static void check_parts(const char* what, const std::vector<part>& parts, uint64_t total) {
  uint64_t end = 0;
  for (size_t k = 0; k < parts.size(); k++) {
    CHECK(parts[k].off % 16 == 0, "%s part %zu at %llu", what, k, (unsigned long long)parts[k].off);
    CHECK(parts[k].off >= end, "%s part %zu at %llu overlaps the one before (ends %llu)", what, k, (unsigned long long)parts[k].off,
          (unsigned long long)end);
    end = parts[k].off + parts[k].bytes;
  }
  CHECK(total >= end, "%s total %llu < end %llu", what, (unsigned long long)total, (unsigned long long)end);
  if (g_failed) return;  // (no write where the arithmetic is wrong already)
  uint8_t* buf = new uint8_t[total];
  memset(buf, 0, total);
  for (size_t k = 0; k < parts.size(); k++) memset(buf + parts[k].off, (int)(k + 1), parts[k].bytes);
  memset(buf + end, 0xff, total - end);  // (the slack behind the last part)
  for (size_t k = 0; k < parts.size(); k++)
    for (uint64_t i = 0; i < parts[k].bytes; i++)
      if (buf[parts[k].off + i] != (uint8_t)(k + 1)) {
        CHECK(false, "%s part %zu byte %llu overwritten", what, k, (unsigned long long)i);
        break;
      }
  delete[] buf;
}

// n_items items whose slice counts and event capacities follow one of three patterns
static void item_counts(int pattern, uint64_t n_items, uint64_t* n_sl, uint64_t* n_ev) {
  *n_sl = *n_ev = 0;
  for (uint64_t i = 0; i < n_items; i++) {
    uint64_t sl = 0, ev = 0;
    if (pattern == 1) sl = 2 * (i % 7) + 1, ev = 2 * (i % 5) + 3;          // odd counts
    if (pattern == 2 && i % 2) sl = 2 * (i % 9) + 1, ev = (i % 4) ? 7 : 0;  // every other item empty, some without events
    *n_sl += sl;
    *n_ev += ev;
  }
}

int main() {
  // {link, slice, result, event, asm_link, asm_call}: the slice is the 16 bytes of grdma_read_slice (part of the C
  // interface; the slice lists are followed by the results without padding); the others as the device structs have
  // them today, and twice with sizes that are no multiples of 16
  const h2_deframe_sizes sizes[] = {{64, 16, 96, 24, 16, 48}, {40, 16, 72, 24, 8, 100}, {8, 16, 4, 12, 24, 36}};
  const uint64_t counts[] = {1, 2, BATCH_MAX};
  for (const h2_deframe_sizes& s : sizes)
    for (uint64_t n : counts)
      for (int pattern = 0; pattern < 3; pattern++) {
        uint64_t n_sl, n_ev;
        item_counts(pattern, n, &n_sl, &n_ev);
        {  // grdma_h2_deframe_batch: table, slice lists, results, event segments
          h2_deframe_sizes plain = s;
          plain.asm_link = plain.asm_call = 0;
          const h2_deframe_block L = h2_deframe_block_layout(plain, n, n_sl, n_ev);
          const uint64_t o_sl = up16(s.link * n);
          const uint64_t o_res = o_sl + s.slice * n_sl;
          const uint64_t o_ev = up16(o_res + s.result * n);
          const uint64_t total = o_ev + s.event * n_ev + 16;
          CHECK(L.tab == 0 && L.slices == o_sl && L.results == o_res && L.events == o_ev && L.total == total,
                "deframe n=%llu pattern=%d", (unsigned long long)n, pattern);
          CHECK(L.asm_tab == o_sl && L.asm_calls == o_sl, "deframe: the assembler's parts are empty");
          check_parts("deframe", {{L.tab, s.link * n}, {L.slices, s.slice * n_sl}, {L.results, s.result * n},
                                  {L.events, s.event * n_ev}}, L.total);
        }
        {  // grdma_h2_deframe_messages_batch: deframe table, assembler table, call blocks, slice lists, results, events
          const h2_deframe_block L = h2_deframe_block_layout(s, n, n_sl, n_ev);
          const uint64_t o_atab = up16(s.link * n);
          const uint64_t o_call = o_atab + up16(s.asm_link * n);
          const uint64_t o_sl = o_call + up16(s.asm_call * n);
          const uint64_t o_res = o_sl + s.slice * n_sl;
          const uint64_t o_ev = up16(o_res + s.result * n);
          const uint64_t total = o_ev + s.event * n_ev + 16;
          CHECK(L.tab == 0 && L.asm_tab == o_atab && L.asm_calls == o_call && L.slices == o_sl && L.results == o_res &&
                    L.events == o_ev && L.total == total,
                "messages n=%llu pattern=%d", (unsigned long long)n, pattern);
          check_parts("messages", {{L.tab, s.link * n}, {L.asm_tab, s.asm_link * n}, {L.asm_calls, s.asm_call * n},
                                   {L.slices, s.slice * n_sl}, {L.results, s.result * n}, {L.events, s.event * n_ev}},
                      L.total);
        }
      }
  // grdma_h2_reply_frame_batch: table, one framer block per item.  (The call had no slack behind the last block; the
  // builder gives every layout the 16 bytes.)
  const uint64_t reply_sizes[][2] = {{8, 216}, {8, 100}, {12, 36}};
  for (const auto& rs : reply_sizes)
    for (uint64_t n : counts) {
      const h2_reply_block L = h2_reply_block_layout(rs[0], rs[1], n);
      const uint64_t o_dev = up16(rs[0] * n);
      const uint64_t total = o_dev + rs[1] * n;
      CHECK(L.tab == 0 && L.devs == o_dev && L.end == total && L.total == total + 16, "reply n=%llu", (unsigned long long)n);
      check_parts("reply", {{L.tab, rs[0] * n}, {L.devs, rs[1] * n}}, L.total);
    }
  // the builder alone: an alignment other than 16
  h2_block b;
  CHECK(b.add(3) == 0 && b.add(5, 64) == 64 && b.add(1, 1) == 69 && b.add(0) == 80 && b.end == 80 && b.total() == 96, "builder");
  printf(g_failed ? "h2_block_host: %d FAILED\n" : "h2_block_host: ok\n", g_failed);
  return g_failed ? 1 : 0;
}
