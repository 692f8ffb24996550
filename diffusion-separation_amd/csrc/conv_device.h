// conv_device.h — the device-side helpers that the convolution kernels, the fused attention block and the GroupNorm finalize
// kernel share word for word: the fixed-point GroupNorm accumulators (write-back, and scale / shift from them), buffer
// addressing, and the GN-affine / hi-lo-split helpers on 16-byte vectors.  Free functions only, all __device__ inline in an
// anonymous namespace.  Included by conv_mfma.hip, conv3x3_ws.hip, conv3x3_small.hip, conv3x3_halo.h (rw / sw / sws),
// attn_fused.hip and norm.hip.
#pragma once

#include "common.h"

namespace {

// ---------------------------------------------------------------- GroupNorm channel-sum accumulators
// [B][C][2] int64 per tensor: slot 0 = sum, slot 1 = sum of squares of a channel over the image, fixed point (2^-24 / 2^-16).
// Producers ADD their tile's totals with integer atomics (associative: the totals are bit-reproducible whatever the order).
#define DS_STAT_SUM_SCALE 16777216.0
#define DS_STAT_SQ_SCALE 65536.0
__device__ inline void ds_stat_add(long long* acc, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)v);
}
// Write-back of a block's total into slot st (0 sum, 1 sum of squares) of a channel's pair `acc`.
__device__ inline __attribute__((always_inline)) void ds_stat_flush(long long* acc, int st, double a) {
  ds_stat_add(acc + st, (long long)llrint(a * (st ? DS_STAT_SQ_SCALE : DS_STAT_SUM_SCALE)));
}
// Scale / shift of one channel from its GROUP's accumulator totals: y = x * sc + sh is gamma * (x - mean) * rstd + beta.
// THE definition of the expression: a consumer may read the table from gn_finalize_acc_kernel or build it in its own
// prologue, and both hold the same bits (tests/test_gn_table_gpu.py).  inv_count = 1 / (pixels * channels per group) as the
// FLOAT of the kernels' argument structs, widened here.  Called by conv3x3_rw / sw / sws.hip and attn_fused.hip; conv_mfma.hip,
// conv3x3_ws.hip, conv3x3_small.hip and norm.hip carry the same lines written out under a comment that points here, because
// their kernels compile to other instruction streams through a function (profiles/conv_device_header_ab.txt).
__device__ inline __attribute__((always_inline)) void ds_gn_affine_from_acc(long long ssum, long long ssq, float inv_count,
                                                                            float eps, float gamma, float beta, float& sc,
                                                                            float& sh) {
  const double mean = (double)ssum * (1.0 / DS_STAT_SUM_SCALE) * (double)inv_count;
  double var = (double)ssq * (1.0 / DS_STAT_SQ_SCALE) * (double)inv_count - mean * mean;
  if (var < 0.0) var = 0.0;
  sc = (float)(1.0 / sqrt(var + (double)eps)) * gamma;
  sh = beta - (float)mean * sc;
}

// ---------------------------------------------------------------- buffer addressing (SRSRC)
// A wave-uniform descriptor + a 32-bit per-lane byte offset + a uniform scalar offset.  Lanes that must not touch memory get
// the offset OOB (>= num_records): the hardware returns 0 for such loads and drops such stores, so halo zero padding, ragged
// tiles and channel tails cost no branches, no exec masking and no zero-initialisation.
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4;
constexpr unsigned OOB = 0x80000000u;
// word 3 (flags) of the descriptor on gfx9 / CDNA: DATA_FORMAT = 32-bit (bit 17 of the word), every other field 0 — a raw
// buffer with stride 0, whose byte offsets are range-checked against num_records
constexpr int RSRC_WORD3 = 0x00020000;
__device__ inline __amdgpu_buffer_rsrc_t rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, RSRC_WORD3);
}
// 16-byte load in the two forms the kernels keep their registers in: ld16 -> uint4 (.x .. .w members), ld16v -> u32x4_t
__device__ inline uint4 ld16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ inline u32x4_t ld16v(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
}
__device__ inline uint2 ld8(__amdgpu_buffer_rsrc_t r, unsigned voff) {
  const u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, 0, 0);
  return make_uint2(v.x, v.y);
}
__device__ inline void st8(__amdgpu_buffer_rsrc_t r, unsigned voff, uint2 d) {
  const u32x2_t v = {d.x, d.y};
  __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, 0, 0);
}
// Block barrier that only orders LDS traffic.  __syncthreads() is a workgroup-scope fence: it drains vmcnt, i.e. it
// would wait for the global prefetch loads issued just before it and serialize them with the barrier.
__device__ inline void sync_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------- GN affine (+ SiLU) on one 16-byte vector
// 8 channels of the 16-bit storage format.  PACKED_HALF (conv3x3_ws.hip only; conv3x3_small.hip and conv_mfma.hip stay on the
// fp32 path ON PURPOSE): in the half-precision build the affine + SiLU run in packed half precision.
template <bool ACT, bool PACKED_HALF = false>
__device__ inline uint4 gn8(const uint4& u, const float* sc, const float* sh) {
#if defined(DS_HALF_F16) && !defined(DS_GN8_F32)
  // half-precision build, round 5: affine + SiLU in packed half precision, 8 instructions per dword (as the register-weight
  // convolution: DESIGN.md section 2 for what it costs in agreement — in front of a convolution, nothing measurable)
  if constexpr (ACT && PACKED_HALF) {
    auto one = [&](unsigned w, int d) __attribute__((always_inline)) {
      const unsigned ps = pack_h2(sc[2 * d], sc[2 * d + 1]), pb = pack_h2(sh[2 * d], sh[2 * d + 1]);
      unsigned z, xx, e, dd, r, o;
      asm("v_pk_fma_f16 %0, %1, %2, %3" : "=v"(z) : "v"(w), "v"(ps), "v"(pb));
      asm("v_pk_mul_f16 %0, %1, %2" : "=v"(xx) : "v"(z), "s"(0xbdc5bdc5u));  // x -log2(e)
      asm("v_exp_f16 %0, %1" : "=v"(e) : "v"(xx));
      asm("v_exp_f16_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1" : "+v"(e) : "v"(xx));
      asm("v_pk_add_f16 %0, %1, %2" : "=v"(dd) : "v"(e), "s"(0x3c003c00u));
      asm("v_rcp_f16 %0, %1" : "=v"(r) : "v"(dd));
      asm("v_rcp_f16_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1" : "+v"(r) : "v"(dd));
      asm("v_pk_mul_f16 %0, %1, %2" : "=v"(o) : "v"(z), "v"(r));
      return o;
    };
    uint4 o;
    o.x = one(u.x, 0); o.y = one(u.y, 1); o.z = one(u.z, 2); o.w = one(u.w, 3);
    return o;
  }
#endif
  float f[8];
  f[0] = h_lo(u.x); f[1] = h_hi(u.x);
  f[2] = h_lo(u.y); f[3] = h_hi(u.y);
  f[4] = h_lo(u.z); f[5] = h_hi(u.z);
  f[6] = h_lo(u.w); f[7] = h_hi(u.w);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = f[j] * sc[j] + sh[j];
    f[j] = ACT ? silu_t<bf16_t>(v) : v;
  }
  uint4 o;
  o.x = pack_h2(f[0], f[1]);
  o.y = pack_h2(f[2], f[3]);
  o.z = pack_h2(f[4], f[5]);
  o.w = pack_h2(f[6], f[7]);
  return o;
}
// 4 fp32 channels
template <bool ACT>
__device__ inline uint4 gn4(const uint4& u, const float* sc, const float* sh) {
  float f[4] = {__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v = f[j] * sc[j] + sh[j];
    f[j] = ACT ? silu_t<float>(v) : v;
  }
  return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
}

// fp32 value = hi + lo with hi, lo bfloat16, round to nearest even both (|error| <= 2^-17 |v|): the operands of the "split" mode,
// in which an fp32 conv runs as three bf16 MFMAs per k-block (hi*hi + hi*lo + lo*hi, fp32 accumulation) instead of eight fp32 MFMAs
__device__ inline void split4(const uint4& v, uint2& hi, uint2& lo) {
  const float f0 = __uint_as_float(v.x), f1 = __uint_as_float(v.y), f2 = __uint_as_float(v.z), f3 = __uint_as_float(v.w);
  hi.x = pack_bf16x2(f0, f1);
  hi.y = pack_bf16x2(f2, f3);
  lo.x = pack_bf16x2(f0 - bf_lo(hi.x), f1 - bf_hi(hi.x));
  lo.y = pack_bf16x2(f2 - bf_lo(hi.y), f3 - bf_hi(hi.y));
}
__device__ inline void split4(const float (&f)[4], u32x2_t& hi, u32x2_t& lo) {
  hi.x = pack_bf16x2(f[0], f[1]);
  hi.y = pack_bf16x2(f[2], f[3]);
  lo.x = pack_bf16x2(f[0] - bf_lo(hi.x), f[1] - bf_hi(hi.x));
  lo.y = pack_bf16x2(f[2] - bf_lo(hi.y), f[3] - bf_hi(hi.y));
}

}  // namespace
