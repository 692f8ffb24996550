// conv3x3_halo.h — what the persistent halo-tile 3x3 convolutions share word for word: conv3x3_rw.hip (register-resident
// weights), conv3x3_sw.hip (streamed weights) and conv3x3_sws.hip (split mode).  Included once by each of them, before its own
// code.  Device side: the tile constants (the buffer helpers and everything else that is not specific to the halo tile come with
// conv_device.h, the per-phase counters of the profiling builds with phase_timing.h).  Host side: the parameter struct of sw and sws
// and what fills it from ConvArgs, the launch tail, the clauses the three ds_conv_*_supported predicates share and the addressing
// preconditions of the kernels' 32-bit offsets and "no tile" pixel indices (halo_addressing_ok).  The kernel BODIES stay apart:
// every function boundary between them moved registers (profiles/experiments/README.md, "Sharing the halo-tile pipeline").
// Everything lives in an anonymous namespace; the profiling builds' launch hooks (halo_env) are host code of these kernels alone.
#pragma once

#include <ctype.h>
#include <stdlib.h>

#include <initializer_list>
#include <type_traits>

#include "conv_device.h"

// ---- profiling build only (the including file defines PT_NAME as rw / rw4 / sw / sws under its -D<X>_TIMING): per-phase cycle
// totals of wave 0, read back through diffsep_<name>_debug_read
#include "phase_timing.h"
#ifdef PT_NAME
// the launch hooks of the profiling builds: DIFFSEP_<RW | SW | SWS>_G (blocks per image: fewer, fatter blocks) and
// DIFFSEP_<..>_DBG (bit 0 = stores fall outside the tensor, bit 1 = loads do; the kernels that read p.dbg), else `dflt`
#define HALO_STR_(a) #a
#define HALO_STR(a) HALO_STR_(a)
static int halo_env(const char* what, int dflt) {
  char n[32];
  snprintf(n, sizeof(n), "DIFFSEP_%s_%s", HALO_STR(PT_NAME), what);
  for (char* c = n + 8; *c != '_'; ++c) *c = (char)toupper(*c);
  const char* v = getenv(n);
  return v ? atoi(v) : dflt;
}
#endif

namespace {

constexpr int TW = 32, HW_ = TW + 2;  // tile width, halo row
constexpr int AROW = 128 + 16;        // 144 B: LDS pitch of a halo pixel's 128-byte chunk line (16 consecutive rows = 16 distinct bank slots)
constexpr int PPL = 8;                // 16-byte pieces (lanes) per pixel: a pixel's chunk is ONE full 128-byte line
constexpr int NT = 256;

// ================================================================ host side

// ---- kernel parameters of the streamed-weight kernels: conv3x3_sw.hip (T = bf16_t) and conv3x3_sws.hip (T = float, the split
// mode's fp32 tensors).  conv3x3_rw.hip has its own RwK (other weight fields); the members of the same name mean the same there.
template <typename T>
struct HaloK {
  const T* x; long x_bs; int ldx; int C1;          // channels [0, C1) from x, [C1, Cin) from x2
  const T* x2; long x2_bs; int ldx2;
  const bf16_t* wfrag; const bf16_t* swfrag;       // fragment-major weights (sw: ds_rw_frag_index, [k-step][Cout / 32][lane][8];
                                                   // sws: ds_sws_frag_index, [k-step][hi | lo][Cout / 32][lane][8])
  unsigned frag_step;                              // bytes of one k-step of the fragment-major copies (sw: Cout / 32 KB; sws: twice that)
  const float* gn_scale; const float* gn_shift;    // [B][Cin] or null
  const long long* gn_acc1; const long long* gn_acc2; const float* gn_gamma; const float* gn_beta;
  int gn_groups; float gn_inv_count; float gn_eps;
  const float* bias; const float* bias_b; int bias_b_ld;
  float out_scale;
  T* y; long y_bs; int ldy;
  long long* stats;
  const T* sx; long sx_bs; int ldsx; int sC1;      // folded skip / residual: raw channels [0, sC1) from sx, the rest from sx2
  const T* sx2; long sx2_bs; int ldsx2;
  int H, W, G, ncb, cout, tiles_x, tiles_per_img;  // G blocks per image and cout block; ncb cout blocks of 128; cout = the layer's
  int dbg;  // profiling builds: bit 0 = stores fall outside the tensor, bit 1 = loads do
};

// the members RwK and HaloK<T> share: sources, GroupNorm operands, bias, scale, output, statistics, image size (the launch tail
// fills in G / tiles_x / tiles_per_img)
template <typename K>
void halo_fill_common(K& k, const ConvArgs& a) {
  using T = std::remove_pointer_t<decltype(k.y)>;
  k.x = reinterpret_cast<const T*>(a.x); k.x_bs = a.x_bs; k.ldx = a.ldx; k.C1 = a.x2 ? a.C1 : a.Cin;
  k.x2 = reinterpret_cast<const T*>(a.x2); k.x2_bs = a.x2_bs; k.ldx2 = a.x2 ? a.ldx2 : a.ldx;
  k.gn_scale = a.gn_scale; k.gn_shift = a.gn_shift;
  k.gn_acc1 = a.gn_acc1; k.gn_acc2 = a.gn_acc2; k.gn_gamma = a.gn_gamma; k.gn_beta = a.gn_beta;
  k.gn_groups = a.gn_groups; k.gn_inv_count = a.gn_inv_count; k.gn_eps = a.gn_eps;
  k.bias = a.bias; k.bias_b = a.bias_b; k.bias_b_ld = a.bias_b_ld;
  k.out_scale = a.out_scale;
  k.y = reinterpret_cast<T*>(a.y); k.y_bs = a.y_bs; k.ldy = a.ldy;
  k.stats = a.stats_acc;
  k.H = a.H; k.W = a.W; k.G = 0; k.tiles_x = 0; k.tiles_per_img = 0;
#ifdef PT_NAME
  k.dbg = halo_env("DBG", 0);
#else
  k.dbg = 0;
#endif
}

// the skip chunks of sw / sws: the folded 1x1 skip on sx (| sx2) against sw_frag, or the residual [B][H][W][Cout] as a folded skip
// against the identity copy ident_frag (exact in the fp32 accumulators), or none.  Returns their channel count.
template <typename T>
int halo_fill_skip(HaloK<T>& k, const ConvArgs& a) {
  k.swfrag = nullptr;
  k.sx = nullptr; k.sx_bs = 0; k.ldsx = 0; k.sC1 = 0; k.sx2 = nullptr; k.sx2_bs = 0; k.ldsx2 = 0;
  if (a.sx) {
    k.sx = reinterpret_cast<const T*>(a.sx); k.sx_bs = a.sx_bs; k.ldsx = a.ldsx; k.sC1 = a.sx2 ? a.sC1 : a.sCin;
    k.sx2 = reinterpret_cast<const T*>(a.sx2); k.sx2_bs = a.sx2_bs; k.ldsx2 = a.sx2 ? a.ldsx2 : a.ldsx;
    k.swfrag = reinterpret_cast<const bf16_t*>(a.sw_frag);
    return a.sCin;
  }
  if (a.res) {
    k.sx = reinterpret_cast<const T*>(a.res); k.sx_bs = a.res_bs; k.ldsx = a.ldr; k.sC1 = a.Cout; k.ldsx2 = a.ldr;
    k.swfrag = reinterpret_cast<const bf16_t*>(a.ident_frag);
    return a.Cout;
  }
  return 0;
}

// ---- the launch tail.  Blocks per image (and cout block) a launch starts from: the compute units over the batch
inline int halo_tiles(const ConvArgs& a, int tile_h) { return (a.H / tile_h) * (a.W / TW); }
inline int halo_blocks_wanted(const ConvArgs& a, int ncb) {
  const int g = ds_num_cus() / (a.B * ncb);
#ifdef PT_NAME
  return halo_env("G", g);
#else
  return g;
#endif
}
// tiles per image, the blocks per image clamped to [1, tiles], the LDS attribute once per device and kernel (KERN is a template
// argument: the statics are per instantiation), launch, check, and the name "family<targs>" for ds_last_conv_kernel()
template <auto KERN, typename K>
int halo_launch(K k, const ConvArgs& a, int tile_h, int g, int ncb, int lds, hipStream_t st, const char* family,
                std::initializer_list<int> targs, int threads = NT) {
  const int tiles = halo_tiles(a, tile_h);
  k.G = g < 1 ? 1 : (g > tiles ? tiles : g);
  k.tiles_x = a.W / TW;
  k.tiles_per_img = tiles;
  DS_FUNC_LDS_ONCE(KERN, lds);
  hipLaunchKernelGGL(KERN, dim3(a.B * ncb * k.G), dim3(threads), lds, st, k);
  DS_LAUNCH_CHECK();
  static char name[64] = {0};
  if (!name[0]) {
    char b[64];
    int n = snprintf(b, sizeof(b), "%s<", family);
    for (int v : targs) n += snprintf(b + n, sizeof(b) - n, "%d,", v);
    b[n - 1] = '>';
    for (int i = n; i >= 0; --i) name[i] = b[i];  // (the first character last: a reader never takes a half-written name)
  }
  ds_set_last_conv_kernel(name);
  return 0;
}

// ---- the clauses the three ds_conv_*_supported share.  kc: channels per chunk; al: elements per 16 bytes
// input: one tensor, or the in-place concat of two split on a chunk boundary; 16-byte pixel pitches
inline bool halo_concat_ok(const ConvArgs& a, int kc, int al) {
  return a.x2 ? a.C1 % kc == 0 && a.C1 > 0 && a.C1 < a.Cin && a.ldx % al == 0 && a.ldx2 % al == 0 : a.ldx % al == 0;
}
// GroupNorm + SiLU from a table or from the producers' accumulators (cpg_max: channels per group the kernel's prologue sums)
inline bool halo_gn_ok(const ConvArgs& a, int cpg_max) {
  if ((a.gn_scale || a.gn_acc1) && !a.gn_act) return false;  // (affine without SiLU does not occur in front of a 3x3 convolution)
  return !a.gn_acc1 || (a.gn_groups > 0 && a.Cin % a.gn_groups == 0 && a.Cin / a.gn_groups <= cpg_max && (!a.x2 || a.gn_acc2));
}
// sources of a folded skip (a.sx != null): as the input's
inline bool halo_skip_split_ok(const ConvArgs& a, int kc, int al) {
  return a.ldsx % al == 0 && (!a.sx2 || (a.sC1 % kc == 0 && a.sC1 > 0 && a.sC1 < a.sCin && a.ldsx2 % al == 0));
}

// ---- addressing preconditions: what the kernels' 32-bit buffer offsets and "no tile" pixel indices assume.  A launch that
// fails them is not given to these kernels (ds_conv_plan falls through to the next route).
// A thread's offset is pixel index x pixel pitch (bytes) + channel offset, the pixel index at most H W (the "no tile" index M
// of sw / sws: the first pixel past the image) + the last halo pixel of a tile of HALO_TH_MAX rows (HALO_TH_MAX W + 33; the
// channel offset, below one pitch, makes it 34).  For EVERY pitch of the launch that product stays below 2^31: bit 31 is the out-of-range
// marker (OOB), and M x pitch — the tensor's size — is then a valid buffer size.  (Every output pitch is >= 128 bytes, so the
// pixel index also fits the 24 bits of the kernels' v_mul_u32_u24.)
// rw_sentinel: conv3x3_rw.hip marks "no tile" with the CONSTANT pixel index 0x3fffff instead of M.  That index has to lie past
// the image (H W + 8 W + 34 <= 0x3fffff), and 0x3fffff + tile offset times the pitch must not wrap past 2^32 back into the
// tensor: every pitch below 1 KB (0x3fffff x 1023 < 2^32 - 4 MB) and the product itself checked.
constexpr int HALO_TH_MAX = 8;  // the tallest tile of the three kernels (each launch function asserts it)
inline bool halo_addressing_ok(const ConvArgs& a, int esz, bool rw_sentinel) {
  long ld = a.ldx > a.ldy ? a.ldx : a.ldy;
  if (a.x2 && a.ldx2 > ld) ld = a.ldx2;
  if (a.sx && a.ldsx > ld) ld = a.ldsx;
  if (a.sx && a.sx2 && a.ldsx2 > ld) ld = a.ldsx2;
  if (a.res && a.ldr > ld) ld = a.ldr;
  const long reach = (long)HALO_TH_MAX * a.W + 34, pix = (long)a.H * a.W + reach, pitch = ld * esz;
  if (pix * pitch >= (1L << 31)) return false;
  if (rw_sentinel && (pitch >= 1024 || pix > 0x3fffff || (0x3fffffL + reach) * pitch >= (1L << 32))) return false;
  return true;
}

}  // namespace
