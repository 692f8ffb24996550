// unit.hip — the unit entry points of the C-ABI: single kernels and single blocks on caller-supplied tensors, for the
// parity tests and the Python operator surface.  No engine state survives a call.
#include "engine_host.h"

// The time embedding of NCSNpp.forward (ncsnpp.py:324-343): GaussianFourierProjection(log t) -> Linear -> SiLU -> Linear, with
// the kernels net_forward launches.  temb [B][4 nf]; workspace >= B * 6 nf floats.
extern "C" int32_t diffsep_time_embedding(const float* t, const float* fourier_w, const float* w1, const float* b1,
                                          const float* w2, const float* b2, float* temb, int32_t B, int32_t nf,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
  DS_CHECK(t && fourier_w && w1 && b1 && w2 && b2 && temb && workspace, "time_embedding: null pointer");
  DS_CHECK(B >= 1 && nf >= 8 && nf % 8 == 0, "time_embedding: bad B / nf");
  DS_CHECK(workspace_bytes >= (int64_t)B * 6 * nf * 4, "time_embedding: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* emb = (float*)workspace;
  float* t1 = emb + (size_t)B * 2 * nf;
  if (ds_launch_fourier(t, fourier_w, emb, B, nf, st)) return 1;
  if (ds_launch_linear(emb, w1, b1, t1, B, 2 * nf, 4 * nf, 0, st)) return 1;
  return ds_launch_linear(t1, w2, b2, temb, B, 4 * nf, 4 * nf, 1, st);
}

// The wide Dense_0 projection of net_forward in isolation: y [B][sum O_i] = act(x) W^T + bias for n_blocks nn.Linear weight
// blocks [O_i][K] stored one after the other in w (block i at row sum_{j<i} O_j), through the two launchers the engine uses —
// ds_launch_dense_transpose per block into the transposed concatenation [K][sum O_i] (arch.hip builds d_dense_w the same way),
// then ds_launch_linear_t.  out_ch_host [n_blocks] (host); bias [sum O_i] or null; workspace >= K * sum O_i floats.
extern "C" int32_t diffsep_dense_projection(const float* x, const float* w, const float* bias, const int32_t* out_ch_host,
                                            int32_t n_blocks, float* y, int32_t B, int32_t K, int32_t silu_in, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
  DS_CHECK(x && w && out_ch_host && y && workspace, "dense_projection: null pointer");
  DS_CHECK(B >= 1 && n_blocks >= 1, "dense_projection: bad B / n_blocks");
  DS_CHECK(K >= 4 && K % 4 == 0 && K <= DS_LINEAR_T_MAX_K, "dense_projection: K must be a multiple of 4 (at most 1024)");  // (before any launch)
  long total = 0;
  for (int i = 0; i < n_blocks; ++i) {
    DS_CHECK(out_ch_host[i] >= 1, "dense_projection: empty weight block");
    total += out_ch_host[i];
  }
  DS_CHECK(total * K < (1L << 31), "dense_projection: weights too large for the transpose's 32-bit index");
  DS_CHECK(workspace_bytes >= total * K * 4, "dense_projection: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* wt = (float*)workspace;
  int off = 0;
  for (int i = 0; i < n_blocks; ++i) {
    if (ds_launch_dense_transpose(w + (long)off * K, wt, out_ch_host[i], K, (int)total, off, st)) return 1;
    off += out_ch_host[i];
  }
  return ds_launch_linear_t(x, wt, bias, y, B, K, (int)total, silu_in, st);
}

extern "C" int32_t diffsep_upfirdn2d(const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx,
                                     int32_t ldy, int32_t up, int32_t dtype, void* stream) {
  DS_CHECK(x && y, "upfirdn2d: null pointer");
  return ds_launch_gn_apply(x, ldx, nullptr, nullptr, C, nullptr, 0, y, ldy, B, H, W, 0, up ? 1 : 2, dtype,
                            (hipStream_t)stream);
}

extern "C" int32_t diffsep_groupnorm_act(const void* x, const float* gamma, const float* beta, void* y, void* xr,
                                         int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx, int32_t ldy,
                                         int32_t ldxr, int32_t groups, float eps, int32_t act, int32_t resample,
                                         int32_t dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  DS_CHECK(x && y && workspace, "groupnorm: null pointer");
  const long wsb = (ds_gn_workspace_bytes(B, H, W, C) + 255) & ~255L;
  DS_CHECK(workspace_bytes >= wsb + 2L * B * C * 4, "groupnorm: workspace too small");
  float* scale = (float*)((char*)workspace + wsb);
  float* shift = scale + (long)B * C;
  hipStream_t st = (hipStream_t)stream;
  if (ds_launch_gn_stats(x, ldx, nullptr, 0, C, B, H, W, C, groups, eps, gamma, beta, workspace, scale, shift, dtype, st))
    return 1;
  return ds_launch_gn_apply(x, ldx, scale, shift, C, y, ldy, xr, ldxr, B, H, W, act, resample, dtype, st);
}

// The GroupNorm-apply / FIR kernels of norm.hip as units on a caller's scale / shift table [B][C] (nullable: the pyramid's pure FIR
// of x into xr), with leading dimensions of the caller's choice.  route = DIFFSEP_GN_AUTO: the dispatch's choice (ds_gn_route,
// what the engine runs); any other DIFFSEP_GN_* code forces that kernel wherever its SHAPE preconditions hold (ds_gn_route_runs)
// and lifts only the dispatch's size thresholds.
static int gn_forced_plan(int route, GnPlan* p) {
  switch (route) {
    case DIFFSEP_GN_APPLY: *p = {GnRoute::APPLY, 0}; return 0;
    case DIFFSEP_GN_BLOCK2X2: *p = {GnRoute::BLOCK2X2, 0}; return 0;
    case DIFFSEP_GN_DOWN_STRIP4: *p = {GnRoute::DOWN_STRIP, 4}; return 0;
    case DIFFSEP_GN_DOWN_STRIP8: *p = {GnRoute::DOWN_STRIP, 8}; return 0;
    case DIFFSEP_GN_DOWN_TILED4: *p = {GnRoute::DOWN_TILED, 4}; return 0;
    case DIFFSEP_GN_DOWN_TILED8: *p = {GnRoute::DOWN_TILED, 8}; return 0;
    case DIFFSEP_GN_UP_TILED: *p = {GnRoute::UP_TILED, 0}; return 0;
  }
  return 1;
}
static int gn_unit_shape(int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx, int32_t ldy, int32_t ldxr, bool has_y, bool has_xr,
                         int32_t mode, int32_t dtype) {
  DS_CHECK(dtype == DS_F32 || dtype == DS_BF16, "gn_apply: bad dtype");
  DS_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0, "gn_apply: bad shape (C a multiple of 8)");
  DS_CHECK(mode >= 0 && mode <= 2 && (mode != 2 || (H % 2 == 0 && W % 2 == 0)), "gn_apply: bad resample mode (FIR down needs even H, W)");
  const int al = dtype == DS_F32 ? 4 : 8;  // (16-byte vectors)
  DS_CHECK(ldx >= C && ldx % al == 0, "gn_apply: ldx must be >= C and a multiple of 16 bytes");
  DS_CHECK(!has_y || (ldy >= C && ldy % al == 0), "gn_apply: ldy must be >= C and a multiple of 16 bytes");
  DS_CHECK(!has_xr || (ldxr >= C && ldxr % al == 0), "gn_apply: ldxr must be >= C and a multiple of 16 bytes");
  return 0;
}
extern "C" int32_t diffsep_gn_apply(const void* x, const float* scale, const float* shift, void* y, void* xr, int32_t B, int32_t H,
                                    int32_t W, int32_t C, int32_t ldx, int32_t ldy, int32_t ldxr, int32_t act, int32_t mode,
                                    int32_t dtype, int32_t route, void* stream) {
  DS_CHECK(x && (scale != nullptr) == (shift != nullptr), "gn_apply: null pointer (scale and shift come together)");
  DS_CHECK((scale != nullptr) == (y != nullptr), "gn_apply: y is written with a table and only with one");
  DS_CHECK(scale || (mode != 0 && xr), "gn_apply: nothing to do");
  DS_CHECK(mode != 0 || !xr, "gn_apply: xr is the resampled raw tensor (mode 1 / 2)");
  if (gn_unit_shape(B, H, W, C, ldx, ldy, ldxr, y != nullptr, xr != nullptr, mode, dtype)) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (route == DIFFSEP_GN_AUTO)
    return ds_launch_gn_apply(x, ldx, scale, shift, C, y, ldy, xr, ldxr, B, H, W, act, mode, dtype, st);
  GnPlan p;
  DS_CHECK(!gn_forced_plan(route, &p), "gn_apply: unknown route code");
  DS_CHECK(ds_gn_route_runs(p.route, mode, scale != nullptr, dtype, H, W, C, ldx, ldy, ldxr, xr != nullptr),
           "gn_apply: the forced kernel's shape preconditions do not hold (2 x 2 blocks: table, up or H % 4 == W % 4 == 0 down; strips: "
           "16-bit, table, down, W % 4 == 0; row tiles: half-precision build, 16-bit, table, down, W % 32 == 0, C % 64 == 0, ld % 8 == 0; "
           "up tiles: table, up, C % 64 == 0)");
  return ds_launch_gn_apply(p, x, ldx, scale, shift, C, y, ldy, xr, ldxr, B, H, W, act, mode, dtype, st);
}
// the route function alone, nothing launched: the name diffsep_gn_apply(route = DIFFSEP_GN_AUTO) would leave in
// diffsep_last_conv_kernel() for this launch on a device of `cus` compute units (<= 0: the current device's); NULL on a bad shape
extern "C" const char* diffsep_gn_route_name(int32_t mode, int32_t affine, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C,
                                             int32_t ldx, int32_t ldy, int32_t ldxr, int32_t has_xr, int32_t cus) {
  if (gn_unit_shape(B, H, W, C, ldx, ldy, ldxr, affine != 0, has_xr != 0, mode, dtype)) return nullptr;
  const GnPlan p = ds_gn_route(mode, affine != 0, dtype, B, H, W, C, ldx, ldy, ldxr, has_xr != 0, cus);
  return ds_gn_kernel_name(p, mode, affine != 0, dtype);
}

// dense-or-strided NHWC view of a caller's tensor
static Tn view(const void* p, int H, int W, int C, int ld) {
  Tn t;
  t.p = const_cast<void*>(p); t.H = H; t.W = W; t.C = C; t.ld = ld;
  return t;
}

extern "C" int32_t diffsep_groupnorm_stats(const void* x, const void* x2, int32_t C1, const float* gamma,
                                           const float* beta, float* scale, float* shift, int32_t B, int32_t H,
                                           int32_t W, int32_t C, int32_t ldx, int32_t ldx2, int32_t groups, float eps,
                                           int32_t dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  DS_CHECK(x && scale && shift && workspace, "groupnorm_stats: null pointer");
  DS_CHECK(workspace_bytes >= ds_gn_workspace_bytes(B, H, W, C), "groupnorm_stats: workspace too small");
  return ds_launch_gn_stats(x, ldx, x2, ldx2, x2 ? C1 : C, B, H, W, C, groups, eps, gamma, beta, workspace, scale, shift,
                            dtype, (hipStream_t)stream);
}

extern "C" int32_t diffsep_conv2d_fused(const void* x, const void* x2, int32_t C1, const float* gn_scale,
                                        const float* gn_shift, int32_t gn_act, const void* w, const float* bias,
                                        const float* bias_b, const void* res, void* y, int32_t B, int32_t H, int32_t W,
                                        int32_t Cin, int32_t Cout, int32_t ksize, int32_t ldx, int32_t ldx2,
                                        int32_t ldr, int32_t ldy, float out_scale, int32_t dtype, int64_t* stats,
                                        int32_t w_chunk, const int64_t* gn_acc1, const int64_t* gn_acc2,
                                        const float* gn_gamma, const float* gn_beta, int32_t gn_groups, void* stream) {
  DS_CHECK(ksize == 1 || ksize == 3, "conv2d: ksize must be 1 or 3");
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.opts = ds_default_opts();
  a.stats_acc = (long long*)stats;
  if (gn_acc1) {
    DS_CHECK(gn_groups > 0 && Cin % gn_groups == 0, "conv2d: bad GroupNorm group count");
    a.gn_acc1 = (const long long*)gn_acc1; a.gn_acc2 = (const long long*)gn_acc2; a.gn_gamma = gn_gamma;
    a.gn_beta = gn_beta; a.gn_groups = gn_groups; a.gn_eps = 1e-6f;
    a.gn_inv_count = gn_inv_count((long)H * W, Cin, gn_groups);
  }
  a.w_chunked = w_chunk;
  Tn xin = view(x, H, W, Cin, ldx);
  xin.p2 = const_cast<void*>(x2); xin.ld2 = ldx2; xin.C1 = C1;
  conv_input(a, xin);
  a.gn_scale = gn_scale; a.gn_shift = gn_shift; a.gn_act = gn_act;
  a.w = w; a.w_bs = 0;
  a.bias = bias; a.bias_b = bias_b; a.bias_b_ld = Cout; a.bias_mode = 0;
  conv_residual(a, view(res, H, W, Cout, ldr));
  a.out_scale = out_scale;
  conv_output(a, view(y, H, W, Cout, ldy));
  a.B = B; a.Cout = Cout; a.taps = ksize == 3 ? 9 : 1;
  const DtypeSplit ds = split_dtype(dtype);
  a.dtype = ds.dtype; a.split = ds.split;
  return ds_launch_conv(a, (hipStream_t)stream);
}
// name (with template arguments) of the kernel the calling thread's last convolution launch ran: lets a test that aims at one
// route fail when the dispatch silently took another
extern "C" const char* diffsep_last_conv_kernel() { return ds_last_conv_kernel(); }
// scale / shift [B][C1 + C2] from the accumulators of one tensor or of the in-place concat of two (the launch the engine puts in
// front of consumers that are not convolutions)
extern "C" int32_t diffsep_gn_finalize_acc(const int64_t* acc1, int32_t C1, const int64_t* acc2, int32_t C2, int32_t B,
                                           int64_t npix, int32_t groups, float eps, const float* gamma, const float* beta,
                                           float* scale, float* shift, void* stream) {
  DS_CHECK(acc1 && scale && shift && C1 > 0 && (acc2 ? C2 > 0 : C2 == 0) && B > 0 && npix > 0, "gn_finalize_acc: bad argument");
  return ds_launch_gn_finalize_acc((const long long*)acc1, C1, (const long long*)acc2, C2, B, npix, groups, eps, gamma, beta,
                                   scale, shift, (hipStream_t)stream);
}
// (the plain convolution: no concat, no GroupNorm, no statistics, row-major weights)
extern "C" int32_t diffsep_conv2d(const void* x, const void* w, const float* bias, const float* bias_b, const void* res,
                                  void* y, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ksize,
                                  int32_t ldx, int32_t ldr, int32_t ldy, float out_scale, int32_t dtype, void* stream) {
  return diffsep_conv2d_fused(x, /*x2, C1*/ nullptr, 0, /*gn_scale, gn_shift, gn_act*/ nullptr, nullptr, 0, w, bias, bias_b, res, y,
                              B, H, W, Cin, Cout, ksize, ldx, /*ldx2*/ 0, ldr, ldy, out_scale, dtype, /*stats, w_chunk*/ nullptr, 0,
                              /*gn_acc1, gn_acc2, gn_gamma, gn_beta, gn_groups*/ nullptr, nullptr, nullptr, nullptr, 0, stream);
}

// The ConvArgs of the two 3x3 unit entries below, as far as they agree: dense NHWC operands (each tensor's leading dimension is its
// channel count) — the input or the in-place concat of two, the optional folded-skip sources, the optional residual, the output —
// B / Cout / taps = 9, the dtype split and the process options.  Weights, GroupNorm, bias, scale and statistics: the caller's.
static ConvArgs conv3x3_dense_args(const void* x, const void* x2, int C1, const void* sx, const void* sx2, int sC1, int sCin,
                                   const void* res, void* y, int B, int H, int W, int Cin, int Cout, int dtype) {
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.opts = ds_default_opts();
  const int c1 = x2 ? C1 : Cin;
  Tn xin = view(x, H, W, Cin, c1);
  xin.p2 = const_cast<void*>(x2); xin.ld2 = Cin - c1; xin.C1 = x2 ? C1 : 0;
  conv_input(a, xin);
  if (sx) {
    const int s1 = sx2 ? sC1 : sCin;
    Tn sin = view(sx, H, W, sCin, s1);
    sin.p2 = const_cast<void*>(sx2); sin.ld2 = sCin - s1; sin.C1 = sx2 ? sC1 : 0;
    conv_skip_input(a, sin);
  }
  conv_residual(a, view(res, H, W, Cout, Cout));
  conv_output(a, view(y, H, W, Cout, Cout));
  a.B = B; a.Cout = Cout; a.taps = 9;
  const DtypeSplit ds = split_dtype(dtype);
  a.dtype = ds.dtype; a.split = ds.split;
  return a;
}

// Unit entry of the streamed-weight 3x3 kernel (conv3x3_sw.hip), whatever the dispatch would have chosen for the shape: dense
// NHWC tensors, weights already in the fragment-major order of diffsep_frag_index (include/diffsep_hip.h).
extern "C" int32_t diffsep_conv3x3_streamed(const void* x, const void* x2, int32_t C1, const float* gn_scale,
                                            const float* gn_shift, const void* w_frag, const float* bias,
                                            const float* bias_b, const void* sx, const void* sx2, int32_t sC1,
                                            int32_t sCin, const void* sw_frag, void* y, int32_t B, int32_t H, int32_t W,
                                            int32_t Cin, int32_t Cout, float out_scale, int32_t dtype, int64_t* stats,
                                            const void* res, const void* ident_frag, const int64_t* gn_acc1,
                                            const int64_t* gn_acc2, const float* gn_gamma, const float* gn_beta,
                                            int32_t gn_groups, void* stream) {
  DS_CHECK(x && w_frag && y, "conv3x3_streamed: null pointer");
  DS_CHECK(!gn_acc1 || (!gn_scale && gn_groups > 0 && Cin % gn_groups == 0 && (!x2 || gn_acc2)), "conv3x3_streamed: bad GroupNorm accumulators");
  DS_CHECK(!res || (ident_frag && !sx), "conv3x3_streamed: a residual needs the identity copy and no skip");
  DS_CHECK(B > 0 && H > 0 && W > 0, "conv3x3_streamed: empty problem");
  DS_CHECK(!x2 || (C1 > 0 && C1 < Cin), "conv3x3_streamed: bad concat split");
  DS_CHECK(!sx || (sw_frag && sCin > 0 && (!sx2 || (sC1 > 0 && sC1 < sCin))), "conv3x3_streamed: bad skip operands");
  ConvArgs a = conv3x3_dense_args(x, x2, C1, sx, sx2, sC1, sCin, res, y, B, H, W, Cin, Cout, dtype);
  a.stats_acc = (long long*)stats;
  a.gn_scale = gn_scale; a.gn_shift = gn_shift; a.gn_act = (gn_scale || gn_acc1) ? 1 : 0;
  if (gn_acc1) {  // GroupNorm of the input from its producers' accumulators, as diffsep_conv2d_fused
    a.gn_acc1 = (const long long*)gn_acc1; a.gn_acc2 = (const long long*)gn_acc2; a.gn_gamma = gn_gamma; a.gn_beta = gn_beta;
    a.gn_groups = gn_groups; a.gn_eps = 1e-6f; a.gn_inv_count = gn_inv_count((long)H * W, Cin, gn_groups);
  }
  a.w = w_frag; a.w_frag = w_frag; a.w_bs = 0;
  a.bias = bias; a.bias_b = bias_b; a.bias_b_ld = Cout; a.bias_mode = 0;
  if (sx) { a.sw = sw_frag; a.sw_frag = sw_frag; }
  a.out_scale = out_scale;
  a.ident_frag = ident_frag;
  // (an image too large for the kernels' 32-bit offsets is no supported shape either: halo_addressing_ok, conv3x3_halo.h)
  if (a.split) {  // fp32 tensors, hi / lo fragment copies: conv3x3_sws.hip
    DS_CHECK(ds_conv_sws_supported(a), "conv3x3_streamed: shape outside the split kernel's instantiations (Cout = 64 / 128 / 256, Cin = 64 .. 256 "
                                       "by 64, W % 32 == 0, H % 8 == 0; skip / residual channels 64 .. 256 by 64 behind GroupNorm; raw input: Cin <= 128)");
    return ds_launch_conv_sws(a, (hipStream_t)stream);
  }
  DS_CHECK(ds_conv_sw_supported(a), "conv3x3_streamed: shape outside the kernel's instantiations (16-bit, Cout = 128 / 256, Cin = 64 .. 256 "
                                    "by 64, W % 32 == 0, H % 4 == 0; a skip needs GroupNorm and Cin = 128; raw input: Cin <= 128; Cout = 64: Cin = 192)");
  return ds_launch_conv_sw(a, ds_conv_plan(a).sw_rows, (hipStream_t)stream);  // (the plan's tile rows, whatever its route)
}
// Unit entry of the register-weight 3x3 kernel (conv3x3_rw.hip), whatever the dispatch would have chosen for the shape, with the
// folded 1x1 skip that diffsep_conv2d_fused has no arguments for: dense NHWC 16-bit tensors, w as in diffsep_conv2d_fused
// ([Cout][9][Cin], or chunk-major with w_chunk), sw [Cout][sCin] row-major.
extern "C" int32_t diffsep_conv3x3_regweight(const void* x, const void* x2, int32_t C1, const float* gn_scale,
                                             const float* gn_shift, const void* w, int32_t w_chunk, const float* bias,
                                             const float* bias_b, const void* sx, const void* sx2, int32_t sC1, int32_t sCin,
                                             const void* sw, const void* res, void* y, int32_t B, int32_t H, int32_t W,
                                             int32_t Cin, int32_t Cout, float out_scale, int32_t dtype, int64_t* stats,
                                             void* stream) {
  DS_CHECK(x && w && y, "conv3x3_regweight: null pointer");
  DS_CHECK(B > 0 && H > 0 && W > 0, "conv3x3_regweight: empty problem");
  DS_CHECK(!x2 || (C1 > 0 && C1 < Cin), "conv3x3_regweight: bad concat split");
  DS_CHECK(!sx || (sw && !res && sCin > 0 && (!sx2 || (sC1 > 0 && sC1 < sCin))), "conv3x3_regweight: bad skip operands");
  ConvArgs a = conv3x3_dense_args(x, x2, C1, sx, sx2, sC1, sCin, res, y, B, H, W, Cin, Cout, dtype);
  a.stats_acc = (long long*)stats;
  a.gn_scale = gn_scale; a.gn_shift = gn_shift; a.gn_act = gn_scale ? 1 : 0;
  a.w = w; a.w_bs = 0; a.w_chunked = w_chunk;
  a.bias = bias; a.bias_b = bias_b; a.bias_b_ld = Cout; a.bias_mode = 0;
  if (sx) { a.sw = sw; a.sw_chunked = 0; }
  a.out_scale = out_scale;
  // (an image too large for the kernel's 32-bit offsets is no supported shape either: halo_addressing_ok, conv3x3_halo.h)
  DS_CHECK(!a.split && ds_conv_rw_supported(a), "conv3x3_regweight: shape outside the kernel's instantiations (16-bit, 64 / 128 -> 64 or "
                                                "128 -> 128, H >= 32, H % 8 == 0, W % 32 == 0; skip: 64 / 128 (/ 192 at 64 -> 64) raw channels)");
  return ds_launch_conv_rw(a, (hipStream_t)stream);
}
extern "C" int64_t diffsep_frag_index(int32_t cout, int32_t tap, int32_t cin, int32_t taps, int32_t Cout) {
  return ds_rw_frag_index(cout, tap, cin, taps, Cout);
}
extern "C" int64_t diffsep_frag_index_split(int32_t cout, int32_t tap, int32_t cin, int32_t taps, int32_t Cout, int32_t plane) {
  return ds_sws_frag_index(cout, tap, cin, taps, Cout, plane);
}

// Unit entry of the fused attention kernel (attn_fused.hip) on caller-supplied operands: x, y dense [B][L][C] 16-bit, the three
// weight matrices in the fragment-major order of diffsep_frag_index(row, 0, column, 1, C) (wqk = Wk^T Wq), GroupNorm of x from its
// producer's accumulators (gn_acc + gamma / beta / groups) or from gn_scale / gn_shift [B][C].
extern "C" int32_t diffsep_attn_fused(const void* x, const int64_t* gn_acc, const float* gn_gamma, const float* gn_beta,
                                      int32_t gn_groups, const float* gn_scale, const float* gn_shift, const void* wqk,
                                      const void* wv, const void* wo, const float* bqk, const float* bv, const float* bo,
                                      void* y, int64_t* stats, int32_t B, int32_t L, int32_t C, void* stream) {
  DS_CHECK(B > 0 && ds_attn_fused_eligible(DS_BF16, C, L), "attn_fused: 128 channels, 16 .. 256 pixels by 16");
  DS_CHECK(!gn_acc || (gn_groups > 0 && C % gn_groups == 0 && C / gn_groups <= 8), "attn_fused: bad GroupNorm group count");
  AttnFusedArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.x_bs = (long)L * C; a.ldx = C;
  a.gn_acc = (const long long*)gn_acc; a.gn_gamma = gn_gamma; a.gn_beta = gn_beta; a.gn_scale = gn_scale; a.gn_shift = gn_shift;
  if (gn_acc) { a.gn_groups = gn_groups; a.gn_inv_count = gn_inv_count(L, C, gn_groups); a.gn_eps = 1e-6f; }
  a.wqk = wqk; a.wv = wv; a.wo = wo; a.bqk = bqk; a.bv = bv; a.bo = bo;
  a.y = y; a.y_bs = (long)L * C; a.ldy = C;
  a.stats = (long long*)stats;
  a.B = B; a.L = L; a.C = C;
  return ds_launch_attn_fused(a, (hipStream_t)stream);
}

extern "C" int32_t diffsep_conv2d_chunk(int32_t ksize, int32_t dtype) { return ds_conv_chunk(ksize == 3 ? 9 : 1, dtype); }

// The general one-tap launch of conv_mfma.hip as a unit: what attention_core and attn_block (engine.hip) assemble by hand for
// Q K^T, P V and V^T.  Y[b, m, n] = ((sum_k A[b | shared, m, k] Bt[b | shared, n, k]) / div_b[b] + bias + res) * out_scale with
// A [M][lda], Bt dense [N][K], res [B][M][ldr], Y [B][M][ldy]; bias along n (mode 0, [N]) or along m (mode 1, [M]).
extern "C" int32_t diffsep_gemm_nt(const void* a, const void* bt, const float* bias, const float* div_b, const void* res, void* y,
                                   int32_t B, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldr, int32_t ldy,
                                   int32_t a_batched, int32_t bt_batched, int32_t bias_mode, float out_scale, int32_t dtype,
                                   void* stream) {
  DS_CHECK(a && bt && y, "gemm_nt: null pointer");
  DS_CHECK(dtype == DS_F32 || dtype == DS_BF16 || dtype == DS_F32_SPLIT, "gemm_nt: bad dtype");
  DS_CHECK(B >= 1 && M >= 1 && N >= 1 && K >= 8 && K % 8 == 0, "gemm_nt: bad shape (K a multiple of 8)");
  DS_CHECK(bias_mode == 0 || bias_mode == 1, "gemm_nt: bias_mode is 0 (along n) or 1 (along m)");
  const int n8 = rup8(N);
  DS_CHECK(lda >= K && lda % 8 == 0, "gemm_nt: lda must be >= K and a multiple of 8");
  DS_CHECK(ldy >= n8 && ldy % 8 == 0, "gemm_nt: ldy must be >= N rounded up to 8 and a multiple of 8");
  DS_CHECK(!res || (ldr >= n8 && ldr % 8 == 0), "gemm_nt: ldr must be >= N rounded up to 8 and a multiple of 8");
  ConvArgs c;
  memset(&c, 0, sizeof(c));
  c.opts = ds_default_opts();
  conv_input(c, view(a, 1, M, K, lda));
  if (!a_batched) c.x_bs = 0;
  c.w = bt; c.w_bs = bt_batched ? (long)N * K : 0;
  c.bias = bias; c.bias_mode = bias_mode; c.div_b = div_b;
  if (res) conv_residual(c, view(res, 1, M, N, ldr));
  c.out_scale = out_scale;
  conv_output(c, view(y, 1, M, N, ldy));
  c.B = B; c.Cout = N; c.taps = 1;
  const DtypeSplit ds = split_dtype(dtype);
  c.dtype = ds.dtype; c.split = ds.split;
  return ds_launch_conv(c, (hipStream_t)stream);
}

extern "C" int32_t diffsep_attention(const void* q, const void* k, const void* vt, void* o, int32_t B, int32_t L,
                                     int32_t C, int32_t ld, int32_t dtype, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  DS_CHECK(q && k && vt && o && workspace, "attention: null pointer");
  DS_CHECK(ld == C, "attention: q/k must be dense [B,L,C] (ld == C)");
  const DtypeSplit ds = split_dtype(dtype);
  const int Lp = rup8(L), esz = ds.dtype == DS_F32 ? 4 : 2;
  const long one = (((long)B * L * Lp * esz) + 255) & ~255L;
  DS_CHECK(workspace_bytes >= 2 * one, "attention: workspace too small");
  return attention_core(view(q, 1, L, C, ld), k, vt, view(o, 1, L, C, ld), B, workspace, (char*)workspace + one, ds.dtype,
                        (hipStream_t)stream, ds.split);
}

// ---- one ResnetBlockBigGANpp / AttnBlockpp through the ENGINE's block code (res_block / attn_block of engine.hip: folded
// Conv_2, GroupNorm from the producer's accumulators, fused FIR resampling, MFMA attention), on caller-supplied
// parameters: the parity tests check the composition against the reference blocks in isolation (layerspp.py:291-323,
// 76-92).  A throw-away one-module engine is built per call (test path, not a hot path) and freed when the call returns.
static std::unique_ptr<diffsep_engine> unit_engine(int dtype, int nf) {
  std::unique_ptr<diffsep_engine> e(new diffsep_engine());
  memset(&e->cfg, 0, sizeof(e->cfg));
  e->cfg.dtype = dtype;
  e->cfg.nf = nf;
  e->opts = ds_default_opts();
  return e;
}
template <typename F>
static int unit_engine_run(diffsep_engine* e, hipStream_t st, F&& body) {
  e->fwd_base = 0;
  e->dry = true;
  e->top = 0;
  if (stats_begin(e, st)) return 1;
  if (body()) { e->dry = false; return 1; }
  e->dry = false;
  const size_t need = e->top + e->stats_need + 8192;
  DS_HIP(hipMalloc((void**)&e->arena, need));
  e->cap = need;
  DS_HIP(hipMemsetAsync(e->arena, 0, need, st));
  e->top = 0;
  if (stats_begin(e, st)) return 1;
  if (body()) return 1;
  DS_HIP(hipStreamSynchronize(st));  // the arena is freed with the engine when the caller returns
  return 0;
}

extern "C" int32_t diffsep_resblock_forward(int32_t in_ch, int32_t out_ch, int32_t up, int32_t down, int32_t temb_dim,
                                            int32_t dtype, const float* params_host, int64_t n_floats, const void* x,
                                            const float* temb, void* y, int32_t B, int32_t H, int32_t W, void* stream) {
  DS_CHECK(params_host && x && temb && y, "resblock_forward: null pointer");
  DS_CHECK(dtype == DS_F32 || dtype == DS_BF16, "resblock_forward: bad dtype");
  DS_CHECK(in_ch % 8 == 0 && out_ch % 8 == 0 && in_ch >= 8 && out_ch >= 8, "resblock_forward: channels must be multiples of 8");
  DS_CHECK(temb_dim >= 4 && temb_dim % 4 == 0, "resblock_forward: temb_dim must be a multiple of 4");
  DS_CHECK(!(up && down) && B >= 1 && H >= 1 && W >= 1 && (!down || (H % 2 == 0 && W % 2 == 0)), "resblock_forward: bad shape");
  const std::unique_ptr<diffsep_engine> owner = unit_engine(dtype, temb_dim / 4);
  diffsep_engine* e = owner.get();
  ArchBuilder(e->arch).res(in_ch, out_ch, up != 0, down != 0, temb_dim);
  if (upload_weights(e, params_host, n_floats, "block_forward: parameter blob")) return 1;
  const Module& m = e->arch.mods[0];
  hipStream_t st = (hipStream_t)stream;
  const int Ho = up ? 2 * H : (down ? H / 2 : H), Wo = up ? 2 * W : (down ? W / 2 : W);
  return unit_engine_run(e, st, [&]() -> int {
    float* proj = e_f32(e, (size_t)B * e->arch.dense_total);
    // Dense_0(act(temb))  layerspp.py:311-312
    if (!e->dry && ds_launch_linear_t(temb, e->d_dense_w, e->d_dense_b, proj, B, temb_dim, e->arch.dense_total, 1, st)) return 1;
    Tn out;
    if (res_block(e, m, view(x, H, W, in_ch, in_ch), proj, B, out, st)) return 1;
    if (!e->dry)
      DS_HIP(hipMemcpyAsync(y, out.p, (size_t)B * Ho * Wo * out_ch * e->esz, hipMemcpyDeviceToDevice, st));
    return 0;
  });
}

extern "C" int32_t diffsep_attnblock_forward(int32_t channels, int32_t dtype, const float* params_host, int64_t n_floats,
                                             const void* x, void* y, int32_t B, int32_t H, int32_t W, void* stream) {
  DS_CHECK(params_host && x && y, "attnblock_forward: null pointer");
  DS_CHECK(dtype == DS_F32 || dtype == DS_BF16, "attnblock_forward: bad dtype");
  DS_CHECK(channels % 8 == 0 && channels >= 8 && B >= 1 && H >= 1 && W >= 1, "attnblock_forward: bad shape");
  const std::unique_ptr<diffsep_engine> owner = unit_engine(dtype, 8);
  diffsep_engine* e = owner.get();
  ArchBuilder(e->arch).attn(channels);
  if (upload_weights(e, params_host, n_floats, "block_forward: parameter blob")) return 1;
  const Module& m = e->arch.mods[0];
  hipStream_t st = (hipStream_t)stream;
  return unit_engine_run(e, st, [&]() -> int {
    Tn out;
    if (attn_block(e, m, view(x, H, W, channels, channels), B, out, st)) return 1;
    if (!e->dry)
      DS_HIP(hipMemcpyAsync(y, out.p, (size_t)B * H * W * channels * e->esz, hipMemcpyDeviceToDevice, st));
    return 0;
  });
}

static float* g_tab = nullptr;
static int g_tab_n = 0;
static int unit_tab(int n_fft, float** tab) {
  if (g_tab_n != n_fft) {
    if (g_tab) hipFree(g_tab);
    g_tab = nullptr;
    g_tab_n = 0;
    if (ds_build_stft_table(n_fft, &g_tab)) return 1;
    g_tab_n = n_fft;
  }
  *tab = g_tab;
  return 0;
}

extern "C" int32_t diffsep_stft_pack_ex(const float* xt, const float* mix, void* y, int32_t B, int32_t S, int64_t T,
                                        int32_t n_fft, int32_t hop, float exponent, float factor, int32_t W, int32_t Cpad,
                                        int32_t centered_shift, int32_t dtype, void* workspace, int64_t workspace_bytes,
                                        void* stream, int32_t split) {
  DS_CHECK(xt && mix && y && workspace, "stft_pack: null pointer");
  DS_CHECK(workspace_bytes >= ds_stft_workspace_bytes(B, S, T, n_fft, hop), "stft_pack: workspace too small");
  float* tab;
  if (unit_tab(n_fft, &tab)) return 1;
  return ds_launch_stft_pack(xt, mix, y, B, S, T, n_fft, hop, exponent, factor, W, Cpad, centered_shift, dtype, tab,
                             (float*)workspace, (hipStream_t)stream, split ? 1 : 0);
}
extern "C" int32_t diffsep_stft_pack(const float* xt, const float* mix, void* y, int32_t B, int32_t S, int64_t T,
                                     int32_t n_fft, int32_t hop, float exponent, float factor, int32_t W, int32_t Cpad,
                                     int32_t centered_shift, int32_t dtype, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  return diffsep_stft_pack_ex(xt, mix, y, B, S, T, n_fft, hop, exponent, factor, W, Cpad, centered_shift, dtype, workspace,
                              workspace_bytes, stream, 0);
}

extern "C" int32_t diffsep_istft_unpack_ex(const void* x, float* out, int32_t B, int32_t S, int64_t T, int32_t n_fft,
                                           int32_t hop, float exponent, float factor, int32_t W, int32_t Cpad,
                                           int32_t dtype, void* workspace, int64_t workspace_bytes, void* stream,
                                           int32_t split, const float* ow, const float* ob, const float* tdiv,
                                           int32_t ow_cin) {
  DS_CHECK(x && out && workspace, "istft_unpack: null pointer");
  DS_CHECK(workspace_bytes >= ds_istft_workspace_bytes(B, S, T, n_fft, hop), "istft_unpack: workspace too small");
  float* tab;
  if (unit_tab(n_fft, &tab)) return 1;
  return ds_launch_istft(x, out, B, S, T, n_fft, hop, exponent, factor, W, Cpad, dtype, tab, (float*)workspace,
                         (hipStream_t)stream, split ? 1 : 0, ow, ob, tdiv, ow_cin);
}
extern "C" int32_t diffsep_istft_unpack(const void* x, float* out, int32_t B, int32_t S, int64_t T, int32_t n_fft,
                                        int32_t hop, float exponent, float factor, int32_t W, int32_t Cpad,
                                        int32_t dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  return diffsep_istft_unpack_ex(x, out, B, S, T, n_fft, hop, exponent, factor, W, Cpad, dtype, workspace, workspace_bytes,
                                 stream, 0, nullptr, nullptr, nullptr, 0);
}


extern "C" int32_t diffsep_sde_sigma_mix(const float* mix, float* sigma_mix, int32_t B, int64_t T, int32_t avg_len,
                                         void* stream) {
  DS_CHECK(mix && sigma_mix, "sde_sigma_mix: null pointer");
  return ds_launch_sigma_mix(mix, sigma_mix, B, T, avg_len, (hipStream_t)stream);
}
extern "C" int32_t diffsep_sde_prior(const diffsep_sde_config* sde, const float* y, const float* z, float* x, int32_t B,
                                     int32_t S, int64_t T, const float* sigma_mix, void* stream) {
  DS_CHECK(sde && y && z && x, "sde_prior: null pointer");
  return ds_launch_sde_prior(to_sdep(sde), y, z, x, B, S, T, sigma_mix, (hipStream_t)stream);
}
extern "C" int32_t diffsep_sde_corrector_update(const diffsep_sde_config* sde, float snr, const float* x, const float* t,
                                                const float* score, const float* z, float* x_out, float* x_mean_out,
                                                int32_t B, int32_t S, int64_t T, const float* sigma_mix, int32_t variant,
                                                void* stream) {
  DS_CHECK(sde && x && t && score && x_out, "sde_corrector_update: null pointer");
  return ds_launch_sde_corrector(to_sdep(sde), snr, x, t, score, z, x_out, x_mean_out, B, S, T, sigma_mix, variant,
                                 (hipStream_t)stream);
}
extern "C" int32_t diffsep_sde_predictor_update(const diffsep_sde_config* sde, int32_t N, const float* x, const float* t,
                                                const float* score, const float* z, float* x_out, float* x_mean_out,
                                                int32_t B, int32_t S, int64_t T, const float* sigma_mix,
                                                int32_t probability_flow, void* stream) {
  DS_CHECK(sde && x && t && score && x_out, "sde_predictor_update: null pointer");
  return ds_launch_sde_predictor(to_sdep(sde), N, x, t, score, z, x_out, x_mean_out, B, S, T, sigma_mix,
                                 probability_flow, (hipStream_t)stream);
}
extern "C" int32_t diffsep_sde_coefficients(const diffsep_sde_config* sde, const float* x, const float* t,
                                            const float* sigma_mix, float* drift_out, float* diffusion_out, int32_t B,
                                            int32_t S, int64_t T, float f_scale, float g_scale, void* stream) {
  DS_CHECK(sde && x && t && drift_out && diffusion_out, "sde_coefficients: null pointer");
  return ds_launch_sde_coeff(to_sdep(sde), x, t, sigma_mix, drift_out, diffusion_out, B, S, T, f_scale, g_scale,
                             (hipStream_t)stream);
}
extern "C" int32_t diffsep_sde_mean(const diffsep_sde_config* sde, const float* x0, const float* t, float* mean_out,
                                    int32_t B, int32_t S, int64_t T, void* stream) {
  DS_CHECK(sde && x0 && t && mean_out, "sde_mean: null pointer");
  return ds_launch_sde_mean(to_sdep(sde), x0, t, mean_out, B, S, T, (hipStream_t)stream);
}
extern "C" int32_t diffsep_sde_std(const diffsep_sde_config* sde, const float* t, const float* sigma_mix, float* std_out,
                                   int32_t B, int32_t S, int64_t T, void* stream) {
  DS_CHECK(sde && t && std_out, "sde_std: null pointer");
  return ds_launch_sde_std(to_sdep(sde), t, sigma_mix, std_out, B, S, T, (hipStream_t)stream);
}
extern "C" int32_t diffsep_sde_mult_std(const float* std, const float* x, float* out, int32_t B, int32_t S, int64_t T,
                                        int32_t per_sample, void* stream) {
  DS_CHECK(std && x && out, "sde_mult_std: null pointer");
  return ds_launch_sde_mult_std(std, x, out, B, S, T, per_sample, (hipStream_t)stream);
}
extern "C" int32_t diffsep_sde_reverse_drift(const float* f, const float* G, const float* score, float* rev_f_out,
                                             int32_t B, int64_t n_per_batch, int32_t g_full, int32_t probability_flow,
                                             void* stream) {
  DS_CHECK(f && G && score && rev_f_out, "sde_reverse_drift: null pointer");
  return ds_launch_sde_reverse(f, G, score, rev_f_out, B, n_per_batch, g_full, probability_flow, (hipStream_t)stream);
}
extern "C" int32_t diffsep_sde_langevin_update(float snr, const float* x, const float* score, const float* z,
                                               float* x_out, float* x_mean_out, int32_t B, int64_t n_per_batch,
                                               void* workspace, int64_t workspace_bytes, void* stream) {
  DS_CHECK(x && score && z && x_out && workspace, "sde_langevin_update: null pointer");
  DS_CHECK(workspace_bytes >= 16 * (int64_t)B + 16, "sde_langevin_update: workspace too small");
  return ds_launch_langevin(snr, x, score, z, x_out, x_mean_out, B, n_per_batch, workspace, (hipStream_t)stream);
}
extern "C" int32_t diffsep_normalize_batch(const float* mix, float* mix_norm, float* mean, float* std, int32_t B,
                                           int64_t T, void* stream) {
  DS_CHECK(mix && mix_norm, "normalize_batch: null pointer");
  return ds_launch_normalize(mix, mix_norm, mean, std, B, T, (hipStream_t)stream);
}
extern "C" int32_t diffsep_scale_output(const float* mix, float* sep, int32_t B, int32_t S, int64_t T, void* stream) {
  DS_CHECK(mix && sep, "scale_output: null pointer");
  return ds_launch_scale_output(mix, sep, B, S, T, (hipStream_t)stream);
}
extern "C" int32_t diffsep_gram(const float* ref, const float* est, double* out, int32_t B, int32_t S, int64_t T,
                                void* stream) {
  DS_CHECK(ref && est && out, "gram: null pointer");
  return ds_launch_gram(ref, est, out, B, S, T, (hipStream_t)stream);
}
extern "C" int32_t diffsep_randn(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream) {
  DS_CHECK(out || n <= 0, "randn: null pointer");  // (an empty tensor has no address: n = 0 draws nothing and launches nothing)
  return ds_launch_randn(out, n, seed, stream_id, (hipStream_t)stream);
}
extern "C" int32_t diffsep_randn_batch(float* out, int32_t B, int32_t S, int64_t T, const uint64_t* seeds,
                                       const int32_t* lengths, uint64_t stream_id, void* stream) {
  DS_CHECK(out && seeds && lengths && B >= 1 && S >= 1 && T >= 1, "randn_batch: bad argument");
  return ds_launch_randn_batch(out, B, S, T, seeds, lengths, stream_id, (hipStream_t)stream);
}
extern "C" int32_t diffsep_convert(const void* src, void* dst, int64_t n, int32_t sd, int32_t dd, void* stream) {
  DS_CHECK(src && dst, "convert: null pointer");
  return ds_launch_convert(src, dst, n, sd, dd, (hipStream_t)stream);
}
