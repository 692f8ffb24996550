// conv3x3_halo.h — what the persistent halo-tile 3x3 convolutions share word for word: conv3x3_rw.hip (register-resident
// weights), conv3x3_sw.hip (streamed weights) and conv3x3_sws.hip (split mode).  Included once by each of them, before its own
// code: the per-phase timing scaffolding of the profiling builds and the tile constants (the buffer helpers and everything else
// that is not specific to the halo tile come with conv_device.h).  The constants live in an anonymous namespace; the profiling
// build's counters (g_<name>_dbg) and read-back function keep the names and external linkage they had in each kernel file.
#pragma once

#include <type_traits>

#include "conv_device.h"

// ---- profiling build only (the including file defines HALO_TIMING as rw / sw / sws): per-phase cycle totals of wave 0,
// read back through diffsep_<name>_debug_read
#ifdef HALO_TIMING
#define HALO_CAT_(a, b, c) a##b##c
#define HALO_CAT(a, b, c) HALO_CAT_(a, b, c)
#define HALO_DBG HALO_CAT(g_, HALO_TIMING, _dbg)
__device__ unsigned long long HALO_DBG[16];
extern "C" int HALO_CAT(diffsep_, HALO_TIMING, _debug_read)(unsigned long long* out, int reset) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(HALO_DBG), sizeof(unsigned long long) * 16);
  if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(HALO_DBG), z, sizeof(z)); }
  return 0;
}
#define RT_DECL unsigned rt_prev = (unsigned)__builtin_readcyclecounter(), rt_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define RT_MARK(i) { unsigned rt_now = (unsigned)__builtin_readcyclecounter(); rt_acc[i] += rt_now - rt_prev; rt_prev = rt_now; }
#define RT_FLUSH if (threadIdx.x == 0) { for (int q = 0; q < 8; ++q) atomicAdd(&HALO_DBG[q], (unsigned long long)rt_acc[q]); atomicAdd(&HALO_DBG[15], 1ull); }
#else
#define RT_DECL
#define RT_MARK(i)
#define RT_FLUSH
#endif

namespace {

constexpr int TW = 32, HW_ = TW + 2;  // tile width, halo row
constexpr int AROW = 128 + 16;        // 144 B: LDS pitch of a halo pixel's 128-byte chunk line (16 consecutive rows = 16 distinct bank slots)
constexpr int PPL = 8;                // 16-byte pieces (lanes) per pixel: a pixel's chunk is ONE full 128-byte line
constexpr int NT = 256;

}  // namespace
