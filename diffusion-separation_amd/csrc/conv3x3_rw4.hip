// conv3x3_rw4.hip — the 4-wave form of the instantiations of conv3x3_rw.hip that run with helper waves (64 -> 64 couts,
// GroupNorm + SiLU, 0 .. 3 skip chunks), behind engine option no_rw_helper: the A/B of the helper form and the reference of
// tests/test_rw_helper_gpu.py.  The same source text compiled a second time — the kernels live in an anonymous namespace, this
// translation unit instantiates only those four and exports one entry, ds_launch_conv_rw4 — because a function boundary around
// the kernel body, which two kernels in one file would need, moves the registers of every instantiation.
#define RW_NO_HELPER
#define RW_FOUR_WAVE_TU
#include "conv3x3_rw.hip"
