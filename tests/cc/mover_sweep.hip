// TEST INFRASTRUCTURE.  The byte movers of csrc/grdma_devfn.h -- wave_copy_tile, wave_copy_tile_g, wave_zero_tile,
// wave_move_tile, tiny_load / tiny_store, plan_tags, plan_tile and the segment-list runner run_plan -- called
// directly, one wave per case, so that a test can compare what they leave in memory with memcpy over the whole of
// two pools (tests/test_zz_gpu_movers.py on the device, tests/test_movers_emu.py under the wave emulator).
// One source for both builds:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared mover_sweep.hip -o libmover_sweep.so
//   clang++ -x c++ -Itests/cc -Itests/cc/emu_include ... -shared mover_sweep.hip -o libmover_sweep_emu.so
// Includes grdma_dev.h and grdma_devfn.h unchanged and nothing else of the product.
//
// A mover that is wrong must damage canary bytes, not leave the allocation: the entries refuse a case or a segment
// whose window is closer than MS_MARGIN bytes to either end of its pool (plans: MS_PLAN_MARGIN, a mis-attributed
// tile lands up to 64 tiles away from its segment).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../grpc-rdma_amd/csrc/grdma_dev.h"
#include "../../grpc-rdma_amd/csrc/grdma_devfn.h"

#define MS_MARGIN (16384ull + 64ull)           // one full tile (the larger one) + 64
#define MS_PLAN_MARGIN (66ull * 16384ull)

enum ms_variant {
  MS_COPY = 0,        // wave_copy_tile
  MS_COPY_NULL = 1,   // ... with src == nullptr
  MS_COPY_G = 2,      // wave_copy_tile_g
  MS_COPY_G_NULL = 3, // ... with src == nullptr
  MS_ZERO = 4,        // wave_zero_tile
  MS_MOVE8 = 5,       // wave_move_tile<GRDMA_PLAN_LD, GRDMA_PLAN_ST, false, 8>
  MS_MOVE16 = 6,      // ... U = 16
  MS_MOVE8_Z = 7,     // wave_move_tile<GRDMA_PLAN_LD_ZERO, GRDMA_PLAN_ST_ZERO, true, 8>
  MS_MOVE16_Z = 8,    // ... U = 16
  MS_TINY = 9,        // tiny_load + tiny_store
  MS_TINY_Z = 10,     // ... with GRDMA_SEG_ZERO_SRC
  MS_NVARIANTS = 11
};

struct ms_case {
  uint32_t variant;
  uint32_t n;
  uint64_t d;  // offset of the destination window in the destination pool
  uint64_t s;  // offset of the source window in the source pool (ignored by the variants without a source)
};

// One wave per case.
__global__ void k_ms_tiles(uint8_t* dpool, uint8_t* spool, const ms_case* cases, uint32_t ncases) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = uni32((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (wave >= ncases) return;
  const ms_case c = cases[wave];
  const uint32_t variant = uni32(c.variant), n = uni32(c.n);
  uint8_t* const dst = dpool + uni64(c.d);
  uint8_t* const src = spool + uni64(c.s);
  switch (variant) {
    case MS_COPY: wave_copy_tile(dst, src, n, lane); break;
    case MS_COPY_NULL: wave_copy_tile(dst, nullptr, n, lane); break;
    case MS_COPY_G: wave_copy_tile_g(dst, src, n, lane); break;
    case MS_COPY_G_NULL: wave_copy_tile_g(dst, nullptr, n, lane); break;
    case MS_ZERO: wave_zero_tile(dst, n, lane); break;
    case MS_MOVE8: wave_move_tile<GRDMA_PLAN_LD, GRDMA_PLAN_ST, false, 8>((uint64_t)dst, (uint64_t)src, n, lane); break;
    case MS_MOVE16: wave_move_tile<GRDMA_PLAN_LD, GRDMA_PLAN_ST, false, 16>((uint64_t)dst, (uint64_t)src, n, lane); break;
    case MS_MOVE8_Z: wave_move_tile<GRDMA_PLAN_LD_ZERO, GRDMA_PLAN_ST_ZERO, true, 8>((uint64_t)dst, (uint64_t)src, n, lane); break;
    case MS_MOVE16_Z: wave_move_tile<GRDMA_PLAN_LD_ZERO, GRDMA_PLAN_ST_ZERO, true, 16>((uint64_t)dst, (uint64_t)src, n, lane); break;
    case MS_TINY:
    case MS_TINY_Z: {
      const grdma_seg sg = {(uint64_t)dst, (uint64_t)src, n, variant == MS_TINY_Z ? GRDMA_SEG_ZERO_SRC : 0ull};
      const uint8_t b = tiny_load(sg, lane);
      tiny_store(sg, b, 0, ~0ull, lane);
      break;
    }
    default: break;
  }
}

// shaped like k_copy
template <bool CONTIG>
__global__ __launch_bounds__(COPY_THREADS) void k_ms_plan(const grdma_plan* plan) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * COPY_THREADS + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * COPY_THREADS) >> 6;
  run_plan<256, CONTIG>(plan, wave, nwaves, lane);
}
// shaped like the inline callers: one plan workgroup runs its own plan
__global__ __launch_bounds__(PLAN_THREADS) void k_ms_plan_inline(const grdma_plan* plan) {
  run_plan<1024, true>(plan, threadIdx.x >> 6, PLAN_THREADS / 64, threadIdx.x & 63);
}

namespace {
struct dev_pools {
  uint8_t *d = nullptr, *s = nullptr;
  void* aux = nullptr;
  ~dev_pools() {
    if (d) (void)hipFree(d);
    if (s) (void)hipFree(s);
    if (aux) (void)hipFree(aux);
  }
};
#define MS_HIP(x)                        \
  do {                                   \
    const hipError_t e_ = (x);           \
    if (e_ != hipSuccess) return -(int64_t)(10000 + (int)e_); \
  } while (0)

bool inside(uint64_t off, uint64_t n, uint64_t pool_len, uint64_t margin) {
  return pool_len >= 2 * margin && off >= margin && off <= pool_len - margin && n <= pool_len - margin - off;
}
uint32_t cap_of(uint32_t variant) {
  switch (variant) {
    case MS_MOVE8: case MS_MOVE8_Z: return 8192;
    case MS_MOVE16: case MS_MOVE16_Z: return 16384;
    case MS_TINY: case MS_TINY_Z: return GRDMA_TINY_MAX;
    default: return 1u << 20;  // the loop movers take any length
  }
}
}  // namespace

// Runs ncases one-wave cases in one launch of `threads` threads per workgroup; both pools come back as they are
// afterwards.  Returns the number of cases run; -1 .. -9 a refused argument, -(10000 + hipError_t) a HIP error.
extern "C" int64_t ms_run_tiles(uint8_t* dpool, uint64_t dlen, uint8_t* spool, uint64_t slen, const ms_case* cases,
                                uint32_t ncases, uint32_t threads) {
  if (ncases == 0) return 0;
  if (threads == 0 || threads > 1024 || (threads & 63)) return -1;
  for (uint32_t i = 0; i < ncases; i++) {
    const ms_case& c = cases[i];
    if (c.variant >= MS_NVARIANTS) return -2;
    if (c.n > cap_of(c.variant)) return -3;  // (a mover's hard capacity: its registers hold no more)
    if (!inside(c.d, c.n, dlen, MS_MARGIN)) return -4;
    if (!inside(c.s, c.n, slen, MS_MARGIN)) return -5;
  }
  dev_pools p;
  MS_HIP(hipMalloc(&p.d, dlen));
  MS_HIP(hipMalloc(&p.s, slen));
  MS_HIP(hipMalloc(&p.aux, sizeof(ms_case) * (size_t)ncases));
  MS_HIP(hipMemcpy(p.d, dpool, dlen, hipMemcpyHostToDevice));
  MS_HIP(hipMemcpy(p.s, spool, slen, hipMemcpyHostToDevice));
  MS_HIP(hipMemcpy(p.aux, cases, sizeof(ms_case) * (size_t)ncases, hipMemcpyHostToDevice));
  const uint32_t per = threads / 64;
  uint8_t *dd = p.d, *ds = p.s;
  const ms_case* dc = static_cast<const ms_case*>(p.aux);
  hipLaunchKernelGGL(k_ms_tiles, dim3((ncases + per - 1) / per), dim3(threads), 0, (hipStream_t)0, dd, ds, dc, ncases);
  MS_HIP(hipGetLastError());
  MS_HIP(hipDeviceSynchronize());
  MS_HIP(hipMemcpy(dpool, p.d, dlen, hipMemcpyDeviceToHost));
  MS_HIP(hipMemcpy(spool, p.s, slen, hipMemcpyDeviceToHost));
  return (int64_t)ncases;
}

// Runs one plan.  kind 0: run_plan<256, true>, 1: run_plan<256, false> (grid workgroups of COPY_THREADS), 2: the inline
// shape, run_plan<1024, true> in one workgroup of PLAN_THREADS.  segs: four words per segment {offset of dst in the
// destination pool, offset of src in the source pool or ~0 for a zero-fill segment, len, flags}; tile_prefix: nsegs + 1
// entries.  The tag window starts at tag_off of the destination (tag_pool 0) or the source pool (1).
// Returns the number of segments; negative as ms_run_tiles.
extern "C" int64_t ms_run_plan(int kind, uint32_t grid, uint8_t* dpool, uint64_t dlen, uint8_t* spool, uint64_t slen,
                               const uint64_t* segs, uint32_t nsegs, const uint32_t* tile_prefix, uint32_t tile_bytes,
                               int tag_pool, uint64_t tag_off, uint64_t tag_mask) {
  if (kind < 0 || kind > 2 || grid == 0 || grid > 4096) return -1;
  if (nsegs == 0 || nsegs > GRDMA_MAX_SEGS) return -2;
  if (tile_bytes != 8192u && tile_bytes != 16384u) return -3;
  if (tag_pool != 0 && tag_pool != 1) return -6;
  if (tag_mask != ~0ull && !inside(tag_off, tag_mask + 1, tag_pool ? slen : dlen, MS_PLAN_MARGIN)) return -7;
  uint64_t total = 0;
  for (uint32_t i = 0; i < nsegs; i++) {
    const uint64_t* g = segs + 4 * (size_t)i;
    if (!inside(g[0], g[2], dlen, MS_PLAN_MARGIN)) return -4;
    if (g[1] != ~0ull && !inside(g[1], g[2], slen, MS_PLAN_MARGIN)) return -5;
    if (tile_prefix[i + 1] < tile_prefix[i]) return -8;
    // (a segment's tiles cover it, no more: the runner computes a tile's length from them)
    if ((uint64_t)(tile_prefix[i + 1] - tile_prefix[i]) != (g[2] + tile_bytes - 1) / tile_bytes) return -8;
    total += g[2];
  }
  if (tile_prefix[0] != 0) return -8;
  dev_pools p;
  MS_HIP(hipMalloc(&p.d, dlen));
  MS_HIP(hipMalloc(&p.s, slen));
  MS_HIP(hipMalloc(&p.aux, sizeof(grdma_plan)));
  grdma_plan* hp = static_cast<grdma_plan*>(calloc(1, sizeof(grdma_plan)));
  if (!hp) return -9;
  hp->nsegs = nsegs;
  hp->ntiles = tile_prefix[nsegs];
  hp->bytes = total;
  hp->tag_base = (uint64_t)(tag_pool ? p.s : p.d) + tag_off;
  hp->tag_mask = tag_mask;
  hp->tile_bytes = tile_bytes;
  for (uint32_t i = 0; i < nsegs; i++) {
    const uint64_t* g = segs + 4 * (size_t)i;
    hp->segs[i] = grdma_seg{(uint64_t)p.d + g[0], g[1] == ~0ull ? 0ull : (uint64_t)p.s + g[1], g[2], g[3]};
  }
  memcpy(hp->tile_prefix, tile_prefix, sizeof(uint32_t) * ((size_t)nsegs + 1));
  const hipError_t e1 = hipMemcpy(p.aux, hp, sizeof(grdma_plan), hipMemcpyHostToDevice);
  free(hp);
  MS_HIP(e1);
  MS_HIP(hipMemcpy(p.d, dpool, dlen, hipMemcpyHostToDevice));
  MS_HIP(hipMemcpy(p.s, spool, slen, hipMemcpyHostToDevice));
  const grdma_plan* dp = static_cast<const grdma_plan*>(p.aux);
  if (kind == 0) hipLaunchKernelGGL((k_ms_plan<true>), dim3(grid), dim3(COPY_THREADS), 0, (hipStream_t)0, dp);
  else if (kind == 1) hipLaunchKernelGGL((k_ms_plan<false>), dim3(grid), dim3(COPY_THREADS), 0, (hipStream_t)0, dp);
  else hipLaunchKernelGGL(k_ms_plan_inline, dim3(1), dim3(PLAN_THREADS), 0, (hipStream_t)0, dp);
  MS_HIP(hipGetLastError());
  MS_HIP(hipDeviceSynchronize());
  MS_HIP(hipMemcpy(dpool, p.d, dlen, hipMemcpyDeviceToHost));
  MS_HIP(hipMemcpy(spool, p.s, slen, hipMemcpyDeviceToHost));
  return (int64_t)nsegs;
}

extern "C" uint64_t ms_margin(int plan) { return plan ? MS_PLAN_MARGIN : MS_MARGIN; }
