// phase_timing.h — the per-phase cycle counters of the profiling builds, once.  Shipped builds define no timing macro: then this
// header declares nothing and every PT_* expands to nothing.
//
// A kernel source that has marks names its counter set, only under its own -D<X>_TIMING macro, before including this header:
//     #ifdef WS_TIMING
//     #define PT_NAME ws          // counters g_ws_dbg, read back through diffsep_ws_debug_read
//     #endif
//     #include "phase_timing.h"
// (PT_READ, if defined beside PT_NAME, names the read-back function instead: conv_mfma.hip's is diffsep_debug_read.)
// Build such a library with `make variant` (csrc/Makefile) and read it with tools/phase_timing.py.
//
// In the kernel:
//     PT_DECL                 once, where timing starts: the previous tick and 12 zeroed accumulators, all 64-bit, per thread
//     PT_MARK(i)              the ticks (__builtin_readcyclecounter) since the previous mark, or since PT_DECL, go to phase i, 0 <= i < 12
//     PT_WAIT                 drains the thread's outstanding vector-memory loads, so that the next mark measures their latency
//     PT_FLUSH                thread 0 adds its accumulators to row 0
//     PT_FLUSH_IF(cond, row)  the thread(s) for which cond holds add theirs to `row` (0 or 1): a second reporting wave
//
// Layout of the counters, PT_ROWS = 2 rows of PT_SLOTS = 16 unsigned long long (the read-back function copies all 32 and, with
// reset != 0, zeroes them):
//     [16 row + 0 .. 11]  ticks of phases 0 .. 11, summed over the blocks that flushed into the row
//     [16 row + 12, 13]   unused
//     [16 row + 14]       wall clock from PT_DECL to the flush (s_memrealtime, 100 MHz), summed likewise
//     [16 row + 15]       number of flushes = blocks
#pragma once

#ifdef PT_NAME
#define PT_CAT_(a, b, c) a##b##c
#define PT_CAT(a, b, c) PT_CAT_(a, b, c)
#define PT_DBG PT_CAT(g_, PT_NAME, _dbg)
#ifndef PT_READ
#define PT_READ PT_CAT(diffsep_, PT_NAME, _debug_read)
#endif
#define PT_SLOTS 16
#define PT_ROWS 2
__device__ unsigned long long PT_DBG[PT_ROWS * PT_SLOTS];
extern "C" int PT_READ(unsigned long long* out, int reset) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(PT_DBG), sizeof(unsigned long long) * PT_ROWS * PT_SLOTS);
  if (reset) { unsigned long long z[PT_ROWS * PT_SLOTS] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(PT_DBG), z, sizeof(z)); }
  return 0;
}
#define PT_DECL unsigned long long pt_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; const unsigned long long pt_wall0 = __builtin_amdgcn_s_memrealtime(); unsigned long long pt_prev = __builtin_readcyclecounter();
#define PT_MARK(i) { const unsigned long long pt_now = __builtin_readcyclecounter(); pt_acc[i] += pt_now - pt_prev; pt_prev = pt_now; }
#define PT_WAIT asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#define PT_FLUSH_IF(cond, row) if (cond) { unsigned long long* pt_row = &PT_DBG[(row) * PT_SLOTS]; for (int pt_q = 0; pt_q < 12; ++pt_q) atomicAdd(&pt_row[pt_q], pt_acc[pt_q]); atomicAdd(&pt_row[14], __builtin_amdgcn_s_memrealtime() - pt_wall0); atomicAdd(&pt_row[15], 1ull); }
#define PT_FLUSH PT_FLUSH_IF(threadIdx.x == 0, 0)
#else
#define PT_DECL
#define PT_MARK(i)
#define PT_WAIT
#define PT_FLUSH_IF(cond, row)
#define PT_FLUSH
#endif
