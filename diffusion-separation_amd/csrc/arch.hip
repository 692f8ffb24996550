// arch.hip — the architecture walk of NCSN++ (models/ncsnpp.py:106-308 ctor), its parameter table in reference state_dict
// order, and the upload of a weight blob: the fp32 copy plus every weight repacked into the layouts the kernels read.
#include "engine_host.h"

int build_arch(const diffsep_model_config& c, Arch& A, int frag_mask) {
  DS_CHECK(c.nf >= 8 && c.nf % 8 == 0, "config: nf must be a positive multiple of 8");
  DS_CHECK(c.num_sources >= 1 && c.num_sources <= 3, "config: num_sources must be 1..3");
  DS_CHECK(c.n_levels >= 1 && c.n_levels <= 8, "config: n_levels must be 1..8");
  DS_CHECK(c.num_res_blocks >= 1, "config: num_res_blocks");
  DS_CHECK(c.n_fft % 2 == 0 && c.n_fft <= 512 && c.hop > 0, "config: n_fft must be even and <= 512");
  A = Arch();
  const int nf = c.nf, channels = 2 * c.num_sources + 2;
  A.chan_in = channels;
  A.chan_out = 2 * c.num_sources;
  A.cpad_in = rup8(channels);
  A.cpad_out = rup8(A.chan_out);
  const int image_size = c.n_fft / 2 + 1;
  ArchBuilder b(A, frag_mask);
  // state_dict order: output_layer is registered before all_modules (ncsnpp.py:104-105 vs :308)
  A.out_w = b.add("output_layer.weight", {A.chan_out, channels, 1, 1});
  A.out_b = b.add("output_layer.bias", {A.chan_out});
  A.pk_out = b.pack(A.chan_out, 1, channels);
  b.fourier(nf);
  b.linear(2 * nf, 4 * nf);
  b.linear(4 * nf, 4 * nf);
  b.conv3(channels, nf);
  std::vector<int> hs_c{nf};
  int in_ch = nf;
  const int L = c.n_levels;
  for (int i = 0; i < L; ++i) {
    const int resl = image_size >> i;
    for (int k = 0; k < c.num_res_blocks; ++k) {
      const int out_ch = nf * c.ch_mult[i];
      b.res(in_ch, out_ch, false, false, 4 * nf);
      in_ch = out_ch;
      if (resl == c.attn_resolution) b.attn(in_ch);
      hs_c.push_back(in_ch);
    }
    if (i != L - 1) {
      b.res(in_ch, in_ch, false, true, 4 * nf);
      b.combine(channels, in_ch);
      hs_c.push_back(in_ch);
    }
  }
  in_ch = hs_c.back();
  b.res(in_ch, in_ch, false, false, 4 * nf);
  b.attn(in_ch);
  b.res(in_ch, in_ch, false, false, 4 * nf);
  for (int i = L - 1; i >= 0; --i) {
    const int resl = image_size >> i;
    for (int k = 0; k < c.num_res_blocks + 1; ++k) {
      const int out_ch = nf * c.ch_mult[i];
      const int skip = hs_c.back();
      hs_c.pop_back();
      b.res(in_ch + skip, out_ch, false, false, 4 * nf, in_ch);
      in_ch = out_ch;
    }
    if (resl == c.attn_resolution) b.attn(in_ch);
    b.gn(in_ch);
    b.conv3(in_ch, channels);
    if (i != 0) b.res(in_ch, in_ch, true, false, 4 * nf);
  }
  DS_CHECK(hs_c.empty(), "internal: skip stack not empty");
  return 0;
}

static diffsep_model_config g_tmp_cfg;
static Arch g_tmp_arch;
static bool g_tmp_valid = false;
static int cached_arch(const diffsep_model_config* cfg, Arch** out) {
  DS_CHECK(cfg != nullptr, "null config");
  if (!g_tmp_valid || memcmp(&g_tmp_cfg, cfg, sizeof(*cfg)) != 0) {
    g_tmp_valid = false;
    if (build_arch(*cfg, g_tmp_arch)) return 1;
    g_tmp_cfg = *cfg;
    g_tmp_valid = true;
  }
  *out = &g_tmp_arch;
  return 0;
}

extern "C" int32_t diffsep_param_count(const diffsep_model_config* cfg) {
  Arch* a;
  if (cached_arch(cfg, &a)) return -1;
  return (int32_t)a->params.size();
}
extern "C" int64_t diffsep_param_total(const diffsep_model_config* cfg) {
  Arch* a;
  if (cached_arch(cfg, &a)) return -1;
  return a->total;
}
extern "C" int32_t diffsep_param_info(const diffsep_model_config* cfg, int32_t idx, char* name, int32_t name_cap,
                                      int64_t shape[4], int32_t* ndim, int64_t* offset) {
  Arch* a;
  if (cached_arch(cfg, &a)) return 1;
  DS_CHECK(idx >= 0 && idx < (int)a->params.size(), "param index out of range");
  const ParamInfo& p = a->params[idx];
  if (name && name_cap > 0) {
    strncpy(name, p.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = p.shape[i];
  if (ndim) *ndim = p.ndim;
  if (offset) *offset = p.off;
  return 0;
}
extern "C" int32_t diffsep_num_frames(const diffsep_model_config* cfg, int64_t T) {
  return 1 + (int32_t)((T + cfg->n_fft - cfg->hop) / cfg->hop);
}
extern "C" int32_t diffsep_padded_frames(const diffsep_model_config* cfg, int64_t T) {
  const int F = diffsep_num_frames(cfg, T);
  return 64 * ((F + 63) / 64);
}

// ------------------------------------------------------------------ weight repack kernel
// dst[o][tap][i] (i < Ipad, zero padded) = src[o*so + i*si + tap*st]; kc > 0: chunk-major dst[i / kc][tap][o][i % kc]
// (one K stage of the conv kernel contiguous in memory -> whole 128-byte lines per request)
template <typename T>
__global__ __launch_bounds__(256) void repack_kernel(const float* __restrict__ src, T* __restrict__ dst, int O, int I,
                                                     int Ipad, int taps, long so, long si, long st, int kc) {
  const long total = (long)O * taps * Ipad;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int i = (int)(idx % Ipad);
    const long r = idx / Ipad;
    const int tap = (int)(r % taps);
    const int o = (int)(r / taps);
    const float v = (i < I) ? src[o * so + i * si + tap * st] : 0.f;
    const long d = kc ? ((((long)(i / kc) * taps + tap) * O + o) * kc + i % kc) : idx;
    Elt<T>::st(dst + d, v);
  }
}
// dst[ds_rw_frag_index(o, tap, i)] = src[o*so + i*si + tap*st]: the register-weight kernel's fragment-major copy (16-bit only)
__global__ __launch_bounds__(256) void repack_frag_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int O, int I,
                                                          int taps, long so, long si, long st) {
  const long total = (long)O * taps * I;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int i = (int)(idx % I);
    const long r = idx / I;
    const int tap = (int)(r % taps), o = (int)(r / taps);
    dst[ds_rw_frag_index(o, tap, i, taps, O)] = f2h(src ? src[o * so + i * si + tap * st] : (o == i ? 1.f : 0.f));  // (null: the identity)
  }
}
// ... and the split mode's: hi = bf16(w), lo = bf16(w - hi) at ds_sws_frag_index(o, tap, i, plane); src == null: the O x O identity
__global__ __launch_bounds__(256) void repack_frag_split_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int O, int I,
                                                                int taps, long so, long si, long st) {
  const long total = (long)O * taps * I;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int i = (int)(idx % I);
    const long r = idx / I;
    const int tap = (int)(r % taps), o = (int)(r / taps);
    const float w = src ? src[o * so + i * si + tap * st] : (o == i ? 1.f : 0.f);
    const uint32_t hi = pack_bf16x2(w, 0.f);
    const uint32_t lo = pack_bf16x2(w - bf_lo(hi), 0.f);
    dst[ds_sws_frag_index(o, tap, i, taps, O, 0)] = (bf16_t)(hi & 0xffffu);
    dst[ds_sws_frag_index(o, tap, i, taps, O, 1)] = (bf16_t)(lo & 0xffffu);
  }
}
// Fused attention block: M[c'][k] = sum_c Wk[c'][c] Wq[k][c] (NIN.W is [in][out]: Wq^T applied to h gives q) in fragment-major
// order, and b'[c'] = sum_c Wk[c'][c] b_q[c] — fp32 sums, one rounding to the storage type (attn_fused.hip)
__global__ __launch_bounds__(256) void attn_fold_qk_kernel(const float* __restrict__ wq, const float* __restrict__ wk,
                                                           const float* __restrict__ bq, bf16_t* __restrict__ m_frag,
                                                           float* __restrict__ b_fold, int Cc) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= Cc * Cc) return;
  const int cp = idx / Cc, k = idx % Cc;
  float a = 0.f;
  for (int c = 0; c < Cc; ++c) a = fmaf(wk[(long)cp * Cc + c], wq[(long)k * Cc + c], a);
  m_frag[ds_rw_frag_index(cp, 0, k, 1, Cc)] = f2h(a);
  if (k == 0) {
    float bb = 0.f;
    for (int c = 0; c < Cc; ++c) bb = fmaf(wk[(long)cp * Cc + c], bq[c], bb);
    b_fold[cp] = bb;
  }
}

// ------------------------------------------------------------------ weight repack (fp32 blob -> engine dtype, kernel layout)
static int repack_weight(diffsep_engine* e, const PRef& src, long pk, int O, int I, int taps, long so, long si, long stp,
                         bool allow_chunk = true, int kc_taps = 0, int c1 = 0) {
  const int dtype = e->cfg.dtype;
  const int Ipad = rup8(I);
  // kc_taps: the kernel that will READ these weights (the fused skip conv is read by the 3x3 kernel)
  const int kc = allow_chunk ? weight_chunk(kc_taps ? kc_taps : taps, I, c1, dtype) : 0;
  const long total = (long)O * taps * Ipad;
  long nb = (total + 255) / 256;
  if (nb > 4096) nb = 4096;
  if (dtype == DS_F32)
    hipLaunchKernelGGL(repack_kernel<float>, dim3(nb), dim3(256), 0, 0, e->d_blob + src.off, (float*)(e->d_pack) + pk, O,
                       I, Ipad, taps, so, si, stp, kc);
  else
    hipLaunchKernelGGL(repack_kernel<bf16_t>, dim3(nb), dim3(256), 0, 0, e->d_blob + src.off, (bf16_t*)(e->d_pack) + pk,
                       O, I, Ipad, taps, so, si, stp, kc);
  DS_LAUNCH_CHECK();
  return 0;
}
static int repack_frag(diffsep_engine* e, const PRef& src, long pf, int O, int I, int taps, long so, long si, long stp) {
  const float* w = src.off >= 0 ? e->d_blob + src.off : nullptr;  // (null: the kernels write the identity)
  if (pf >= 0 && e->cfg.dtype == DS_F32 && e->split && ds_sws_frag_shape(taps, I, O)) {  // hi / lo planes: 2 x 2 bytes per weight = one slot
    hipLaunchKernelGGL(repack_frag_split_kernel, dim3(cdiv((long)O * taps * I, 256)), dim3(256), 0, 0, w,
                       (bf16_t*)((float*)(e->d_pack) + pf), O, I, taps, so, si, stp);
    DS_LAUNCH_CHECK();
    return 0;
  }
  if (pf < 0 || e->cfg.dtype != DS_BF16) return 0;
  hipLaunchKernelGGL(repack_frag_kernel, dim3(cdiv((long)O * taps * I, 256)), dim3(256), 0, 0, w,
                     (bf16_t*)(e->d_pack) + pf, O, I, taps, so, si, stp);
  DS_LAUNCH_CHECK();
  return 0;
}
static int repack_module(diffsep_engine* e, const Module& m) {
  int rc = 0;
  switch (m.kind) {
    case MK_CONV3: rc |= repack_weight(e, m.w0, m.pk0, m.out_ch, m.in_ch, 9, (long)m.in_ch * 9, 9, 1); break;
    case MK_COMBINE: rc |= repack_weight(e, m.w0, m.pk0, m.out_ch, m.in_ch, 1, m.in_ch, 1, 0); break;
    case MK_RES:
      rc |= repack_weight(e, m.conv0_w, m.pk0, m.out_ch, m.in_ch, 9, (long)m.in_ch * 9, 9, 1, true, 0, m.in_c1);
      rc |= repack_weight(e, m.conv1_w, m.pk1, m.out_ch, m.out_ch, 9, (long)m.out_ch * 9, 9, 1);
      if (m.has_conv2)
        rc |= repack_weight(e, m.conv2_w, m.pk2, m.out_ch, m.in_ch, 1, m.in_ch, 1, 0, true, fuse_skip(m) ? 9 : 0, m.in_c1);
      rc |= repack_frag(e, m.conv0_w, m.pf0, m.out_ch, m.in_ch, 9, (long)m.in_ch * 9, 9, 1);
      rc |= repack_frag(e, m.conv1_w, m.pf1, m.out_ch, m.out_ch, 9, (long)m.out_ch * 9, 9, 1);
      if (m.has_conv2) rc |= repack_frag(e, m.conv2_w, m.pf2, m.out_ch, m.in_ch, 1, m.in_ch, 1, 0);
      rc |= repack_frag(e, PRef(), m.pf_id, m.out_ch, m.out_ch, 1, 0, 0, 0);  // (no source: the identity)
      if (m.pf0a >= 0) {  // the halves of a cat(128, 128) block (channel offset 128 in the second)
        PRef w0b = m.conv0_w, w2b = m.conv2_w;
        w0b.off += 128L * 9;
        w2b.off += 128;
        rc |= repack_frag(e, m.conv0_w, m.pf0a, m.out_ch, 128, 9, (long)m.in_ch * 9, 9, 1);
        rc |= repack_frag(e, w0b, m.pf0b, m.out_ch, 128, 9, (long)m.in_ch * 9, 9, 1);
        rc |= repack_frag(e, m.conv2_w, m.pf2a, m.out_ch, 128, 1, m.in_ch, 1, 0);
        rc |= repack_weight(e, w2b, m.pk2b, m.out_ch, 128, 1, m.in_ch, 1, 0);
      }
      // Dense_0.weight [out][temb dim] -> columns [temb_off, temb_off + out) of the transposed concatenation
      // [temb dim][dense_total] (ds_launch_linear_t)
      rc |= ds_launch_dense_transpose(e->d_blob + m.dense_w.off, e->d_dense_w, m.out_ch, (int)(m.dense_w.numel / m.out_ch),
                                      e->arch.dense_total, m.temb_off, 0);
      DS_HIP(hipMemcpy(e->d_dense_b + m.temb_off, e->d_blob + m.dense_b.off, (size_t)m.dense_b.numel * 4,
                       hipMemcpyDeviceToDevice));
      break;
    case MK_ATTN:  // NIN.W is [in][out] (layers.py:678-689): packed as [out][in]
      // (the V projection is the A operand of its GEMM: it stays row-major)
      for (int i = 0; i < 4; ++i)
        rc |= repack_weight(e, m.nin_w[i], m.pk_nin[i], m.in_ch, m.in_ch, 1, 1, m.in_ch, 0, i != 2);
      // fused attention kernel: NIN.W is [in][out]; rows of the fragment-major copies of Wv / Wo = outputs ([out][in]); the
      // query and key projections are folded into one matrix and one bias vector
      for (int i = 2; i < 4; ++i) rc |= repack_frag(e, m.nin_w[i], m.pf_nin[i], m.in_ch, m.in_ch, 1, 1, m.in_ch, 0);
      if (m.pf_nin[0] >= 0 && e->cfg.dtype == DS_BF16 && e->d_attn_b) {
        hipLaunchKernelGGL(attn_fold_qk_kernel, dim3(cdiv((long)m.in_ch * m.in_ch, 256)), dim3(256), 0, 0, e->d_blob + m.nin_w[0].off,
                           e->d_blob + m.nin_w[1].off, e->d_blob + m.nin_b[0].off, (bf16_t*)(e->d_pack) + m.pf_nin[0],
                           e->d_attn_b + m.ab_off, m.in_ch);
        DS_LAUNCH_CHECK();
      }
      break;
    default: break;
  }
  return rc;
}

int upload_weights(diffsep_engine* e, const float* weights_host, int64_t n_floats, const char* what) {
  const Arch& A = e->arch;
  if (n_floats != A.total) {
    ds_set_error(std::string(what) + " has " + std::to_string(n_floats) + " floats, expected " + std::to_string(A.total));
    return 1;
  }
  const int temb_dim = 4 * e->cfg.nf;
  e->esz = e->cfg.dtype == DS_F32 ? 4 : 2;
  DS_HIP(hipMalloc((void**)&e->d_blob, (size_t)A.total * 4));
  DS_HIP(hipMemcpy(e->d_blob, weights_host, (size_t)A.total * 4, hipMemcpyHostToDevice));
  DS_HIP(hipMalloc((void**)&e->d_pack, (size_t)A.pack_total * e->esz + 256));
  DS_HIP(hipMemset(e->d_pack, 0, (size_t)A.pack_total * e->esz + 256));
  // (+ 1: an engine of one attention block has no Dense_0 at all)
  DS_HIP(hipMalloc((void**)&e->d_dense_w, (size_t)(A.dense_total + 1) * (temb_dim + 1) * 4));
  DS_HIP(hipMalloc((void**)&e->d_dense_b, (size_t)(A.dense_total + 1) * 4));
  if (A.attn_bias_total) DS_HIP(hipMalloc((void**)&e->d_attn_b, (size_t)A.attn_bias_total * 4));
  int rc = 0;
  if (A.pk_out >= 0) rc = repack_weight(e, A.out_w, A.pk_out, A.chan_out, A.chan_in, 1, A.chan_in, 1, 0);
  for (const Module& m : A.mods) rc |= repack_module(e, m);
  if (rc) return 1;
  DS_HIP(hipDeviceSynchronize());
  return 0;
}
