// The layout of the batch block of grdma_h2_calls_step_batch (grpc-rdma_amd/csrc/grdma_h2_block.h: h2_calls_block_layout)
// on the host: [table | one call block per item | eight result words per item] for every count from 1 to
// GRDMA_H2_BATCH_MAX items, the struct sizes as the device has them today and twice with sizes that are no multiples of 16
// -- against the offset arithmetic written out again below.  Every part is then written end to end into a heap buffer of
// exactly `total` bytes, the result words item by item as the finish launch indexes them: built with
// -fsanitize=address,undefined (tests/test_h2_calls_block_host.py) an overrun ends the program.
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

int main() {
  // {link, call}: h2c_link and h2c_call of csrc/grdma_h2_calls.h, then sizes that are no multiples of 16
  const uint64_t sizes[][2] = {{24, 136}, {20, 100}, {8, 4}};
  for (const auto& s : sizes)
    for (uint64_t n = 1; n <= BATCH_MAX; n++) {
      const h2_calls_block L = h2_calls_block_layout(s[0], s[1], n);
      const uint64_t o_call = up16(s[0] * n);
      const uint64_t o_res = up16(o_call + s[1] * n);
      const uint64_t total = o_res + 64 * n + 16;
      CHECK(L.tab == 0 && L.calls == o_call && L.results == o_res && L.total == total, "calls n=%llu", (unsigned long long)n);
      CHECK(L.calls % 16 == 0 && L.results % 16 == 0 && L.calls >= s[0] * n && L.results >= L.calls + s[1] * n && L.total >= L.results + 64 * n,
            "calls n=%llu: aligned, in order, inside the total", (unsigned long long)n);
      if (g_failed) continue;  // (no write where the arithmetic is wrong already)
      // what goes up is [0, results): the host image; the device block is `total` bytes
      uint8_t* up = new uint8_t[L.results];
      memset(up, 0, L.results);
      uint8_t* dev = new uint8_t[L.total];
      memset(dev, 0, L.total);
      for (uint64_t i = 0; i < n; i++) {
        memset(up + L.tab + s[0] * i, 1, s[0]);
        memset(up + L.calls + s[1] * i, 2, s[1]);
      }
      memcpy(dev, up, L.results);  // the one copy up
      for (uint64_t i = 0; i < n; i++) memset(dev + L.results + 64 * i, 4, 64);  // the finish's eight words of item i
      memset(dev + L.results + 64 * n, 0xff, L.total - (L.results + 64 * n));  // (the slack behind the last part)
      std::vector<uint8_t> down(64 * n);
      memcpy(down.data(), dev + L.results, 64 * n);  // the one copy down
      bool whole = true;
      for (uint64_t i = 0; i < s[0] * n; i++) whole = whole && dev[L.tab + i] == 1;
      for (uint64_t i = 0; i < s[1] * n; i++) whole = whole && dev[L.calls + i] == 2;
      for (uint64_t i = 0; i < 64 * n; i++) whole = whole && down[i] == 4;
      CHECK(whole, "calls n=%llu: a part was overwritten", (unsigned long long)n);
      delete[] dev;
      delete[] up;
    }
  printf(g_failed ? "h2_calls_block_host: %d FAILED\n" : "h2_calls_block_host: ok\n", g_failed);
  return g_failed ? 1 : 0;
}
