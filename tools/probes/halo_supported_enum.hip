// halo_supported_enum.hip — host program, no GPU: do two builds of the library accept the same launches on the three persistent
// halo-tile 3x3 kernels?  It loads both libraries, calls ds_conv_rw_supported / ds_conv_sw_supported / ds_conv_sws_supported of
// each on an enumeration of ConvArgs (Cout, Cin, concat split, skip / residual, GroupNorm mode, image, pitches, layouts, null
// operands) and requires, case by case,
//     new(a) == old(a) && addressing(a)
// where addressing(a) is written out below from the kernels' preconditions, independently of conv3x3_halo.h.  A second sweep
// walks image sizes and pitches across the addressing bounds themselves.
//   hipcc --offload-arch=gfx950 -std=c++17 -I diffusion-separation_amd/csrc tools/probes/halo_supported_enum.hip -ldl -o halo_enum
//   ./halo_enum <old libdiffsep_hip.so> <new libdiffsep_hip.so>        (exit status 1 on any mismatch)
#include <dlfcn.h>
#include <string.h>

#include "common.h"

typedef bool (*pred_t)(const ConvArgs&);
static const char* SYM[3] = {"_Z20ds_conv_rw_supportedRK8ConvArgs", "_Z20ds_conv_sw_supportedRK8ConvArgs", "_Z21ds_conv_sws_supportedRK8ConvArgs"};
static const char* KER[3] = {"rw", "sw", "sws"};

// every pitch the launch uses; (H W + 8 W + 34) x pitch bytes < 2^31; rw: pitch < 1 KB, H W + 8 W + 34 <= 0x3fffff and the constant
// "no tile" index plus a tile, times the pitch, below 2^32
static bool addressing(const ConvArgs& a, int kernel) {
  const long esz = a.dtype == DS_F32 ? 4 : 2;
  const long lds[6] = {a.ldx, a.x2 ? a.ldx2 : 0, a.sx ? a.ldsx : 0, (a.sx && a.sx2) ? a.ldsx2 : 0, a.res ? a.ldr : 0, a.ldy};
  const long pix = (long)a.H * a.W + 8L * a.W + 34;
  for (long ld : lds) {
    if (pix * ld * esz >= 2147483648L) return false;
    if (kernel == 0 && (ld * esz >= 1024 || (0x3fffffL + 8L * a.W + 34) * ld * esz >= 4294967296L)) return false;
  }
  return kernel != 0 || pix <= 0x3fffff;
}

static pred_t P[2][3];
static long n_cases = 0, n_old[3], n_new[3], n_addr[3], n_bad = 0;
static void check(const ConvArgs& a) {
  ++n_cases;
  for (int k = 0; k < 3; ++k) {
    const bool o = P[0][k](a), n = P[1][k](a), ad = addressing(a, k);
    n_old[k] += o; n_new[k] += n; n_addr[k] += o && !ad;
    if (n != (o && ad) && ++n_bad <= 20)
      fprintf(stderr, "MISMATCH %s: old %d new %d addressing %d  Cout %d Cin %d C1 %d x2 %d sx %d sCin %d sC1 %d sx2 %d res %d gn %d/%d/%d act %d groups %d "
              "H %d W %d ld %d %d %d %d %d %d dtype %d split %d\n", KER[k], o, n, ad, a.Cout, a.Cin, a.C1, !!a.x2, !!a.sx, a.sCin, a.sC1, !!a.sx2, !!a.res,
              !!a.gn_scale, !!a.gn_acc1, !!a.gn_acc2, a.gn_act, a.gn_groups, a.H, a.W, a.ldx, a.ldx2, a.ldsx, a.ldsx2, a.ldr, a.ldy, a.dtype, a.split);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <old library> <new library>\n", argv[0]); return 2; }
  for (int l = 0; l < 2; ++l) {
    void* h = dlopen(argv[1 + l], RTLD_NOW | RTLD_LOCAL);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
    for (int k = 0; k < 3; ++k)
      if (!(P[l][k] = (pred_t)dlsym(h, SYM[k]))) { fprintf(stderr, "%s: no %s\n", argv[1 + l], SYM[k]); return 2; }
  }
  static char buf[16];  // (the predicates test pointers for null only)
  void* const p = buf;
  const float* const pf = reinterpret_cast<const float*>(buf);
  const long long* const pl = reinterpret_cast<const long long*>(buf);

  // ---- sweep 1: shapes.  Dense operands (each pitch = its channel count) and, one at a time, the variations listed under `var`
  const int HW[][2] = {{4, 32}, {8, 32}, {12, 64}, {24, 32}, {32, 32}, {40, 64}, {64, 48}, {32, 16}};
  const int COUT[] = {32, 64, 128, 192, 256, 512};
  for (int split = 0; split < 2; ++split)
    for (int Cout : COUT)
      for (int Cin = 0; Cin <= 576; Cin += 32)
        for (int xv = 0; xv < 4; ++xv)          // input: one tensor | concat split at 32, 64, Cin - 64
          for (int sv = 0; sv < 2 + 19 * 3; ++sv)  // none | residual | skip on 0 .. 576 channels: one tensor, split at 32, at 64
            for (int gv = 0; gv < 11; ++gv)       // none | table + SiLU | table alone | accumulators: 4, 8, 16, 32 per group x (acc2 | not)
              for (const auto& hw : HW)
                for (int var = 0; var < 18; ++var) {
                  ConvArgs a;
                  memset(&a, 0, sizeof(a));
                  a.dtype = split ? DS_F32 : DS_BF16; a.split = split; a.taps = 9; a.B = 2; a.H = hw[0]; a.W = hw[1];
                  a.Cin = Cin; a.Cout = Cout; a.out_scale = 1.f;
                  a.x = p; a.w = p; a.w_frag = p; a.y = p; a.ident_frag = p; a.ldx = Cin; a.ldy = Cout;
                  if (xv) { a.x2 = p; a.C1 = xv == 1 ? 32 : xv == 2 ? 64 : Cin - 64; a.ldx = a.C1; a.ldx2 = Cin - a.C1; }
                  if (sv == 1) { a.res = p; a.ldr = Cout; }
                  if (sv >= 2) {
                    const int s = sv - 2;
                    a.sx = p; a.sw = p; a.sw_frag = p; a.sCin = (s / 3) * 32; a.ldsx = a.sCin;
                    if (s % 3) { a.sx2 = p; a.sC1 = s % 3 == 1 ? 32 : 64; a.ldsx = a.sC1; a.ldsx2 = a.sCin - a.sC1; }
                  }
                  if (gv == 1 || gv == 2) { a.gn_scale = pf; a.gn_shift = pf; a.gn_act = gv == 1; }
                  if (gv >= 3) {
                    const int cpg = 4 << ((gv - 3) / 2);
                    a.gn_acc1 = pl; a.gn_acc2 = ((gv - 3) & 1) ? pl : nullptr; a.gn_act = 1; a.gn_groups = Cin / cpg; a.gn_inv_count = 1.f; a.gn_eps = 1e-6f;
                  }
                  switch (var) {
                    case 0: break;
                    case 1: a.w_chunked = 32; break;
                    case 2: a.w_chunked = 16; break;
                    case 3: a.sw_chunked = 16; break;
                    case 4: a.sw_chunked = 24; break;
                    case 5: a.sw_chunked = 8; break;
                    case 6: a.w_frag = nullptr; break;
                    case 7: a.sw_frag = nullptr; break;
                    case 8: a.ident_frag = nullptr; break;
                    case 9: a.sw = nullptr; break;
                    case 10: a.bias_mode = 1; break;
                    case 11: a.div_b = pf; break;
                    case 12: a.w_bs = 64; break;
                    case 13: a.ldx += 4; a.ldsx += 4; break;                   // 16-byte pitches in fp32, not in 16 bits
                    case 14: a.ldx2 += 2; a.ldsx2 += 2; a.ldr += 2; break;   // in neither
                    case 15: a.ldy = 512; break;                               // 1 KB (16-bit) / 2 KB output pitch
                    case 16: a.ldsx = 512; a.ldr = 520; break;                // wide skip / residual pitch
                    case 17: a.ldy = Cout - 8; a.res = p; a.ldr = Cout - 8; a.sx = nullptr; break;  // pitch below Cout
                  }
                  check(a);
                }
  const long n1 = n_cases;
  printf("sweep 1 (shapes): %ld cases\n", n1);
  for (int k = 0; k < 3; ++k) printf("  %-3s accepted: old %ld, new %ld; refused for addressing alone: %ld\n", KER[k], n_old[k], n_new[k], n_addr[k]);

  // ---- sweep 2: the addressing bounds.  One accepted layer per kernel (with a 192-channel folded skip where the kernel has one),
  // W = 32 .. 16384, H around every multiple of 512 (across H W + 8 W + 34 = 0x3fffff and pix x pitch = 2^31), every pitch in turn widened
  long o0[3], n0[3], a0[3];
  for (int k = 0; k < 3; ++k) { o0[k] = n_old[k]; n0[k] = n_new[k]; a0[k] = n_addr[k]; }
  for (int ker = 0; ker < 3; ++ker)
    for (int W : {32, 2048, 4096, 16384})
      for (int hb = 0; hb <= 16384; hb += 512)
       for (int H : {hb - 16, hb - 8, hb, hb + 32, hb + 40})  // (the bounds lie 8 W + 34 pixels = 8.x rows below a power of two)
        if (H > 0) for (int which = 0; which < 6; ++which)     // the pitch that is widened: x, x2, sx, sx2, res, y
          for (int ld : {0, 128, 256, 504, 512, 1024, 4096}) {  // 0: dense
            ConvArgs a;
            memset(&a, 0, sizeof(a));
            a.dtype = ker == 2 ? DS_F32 : DS_BF16; a.split = ker == 2; a.taps = 9; a.B = 1; a.H = H; a.W = W; a.out_scale = 1.f;
            a.x = p; a.w = p; a.w_frag = p; a.y = p; a.ident_frag = p; a.gn_scale = pf; a.gn_shift = pf; a.gn_act = 1;
            a.Cout = ker == 1 ? 128 : 64; a.Cin = ker == 1 ? 128 : 64; a.ldx = a.Cin; a.ldy = a.Cout;
            if (which == 1) { a.Cin = 128; a.x2 = p; a.C1 = 64; a.ldx = 64; a.ldx2 = 64; }
            if (which == 2 || which == 3) { a.sx = p; a.sw = p; a.sw_frag = p; a.sCin = ker == 1 ? 256 : 192; a.ldsx = a.sCin; }
            if (which == 3) { a.sx2 = p; a.sC1 = 64; a.ldsx = 64; a.ldsx2 = a.sCin - 64; }
            if (which == 4) { a.res = p; a.ldr = a.Cout; }
            int* const tgt[6] = {&a.ldx, &a.ldx2, &a.ldsx, &a.ldsx2, &a.ldr, &a.ldy};
            if (ld && ld >= *tgt[which]) *tgt[which] = ld;
            check(a);
          }
  printf("sweep 2 (addressing bounds): %ld cases\n", n_cases - n1);
  for (int k = 0; k < 3; ++k)
    printf("  %-3s accepted: old %ld, new %ld; refused for addressing alone: %ld\n", KER[k], n_old[k] - o0[k], n_new[k] - n0[k], n_addr[k] - a0[k]);
  printf("mismatches (new != old && addressing): %ld\n", n_bad);
  return n_bad ? 1 : 0;
}
