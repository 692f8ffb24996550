// warm_start.hip — from another separator's estimates to the state the sampler starts from at an intermediate time
// (diffsep_warm_start -> x_init of diffsep_pc_sample_from).  The reference has every piece and no such call: the forward
// marginal x_t ~ N(mean_t(x0), Sigma_t) is SDE.marginal_prob (sdes/sdes.py:322-324; PriorMixSDE :515-532), which its training
// draws from in sample_prior (pl_model.py:179-247), on targets normalised by normalize_batch((mix, tgt)) (pl_model.py:81-88).
// Two launches per call, nothing read back, no floating-point atomics:
//   warm_fit_kernel    (scale = ls) block (share, b): float64 partial sums over the utterance's own n = lengths[b] samples of the
//                      Gram matrix of the estimates G[i][j] = sum_t e_i e_j and of their products with the RAW mixture
//                      r[i] = sum_t e_i y (products of two floats are exact in float64), block totals in the fixed order of
//                      reduce_device.h.  The time axis is cut into kWarmParts contiguous shares of warm_share(n) samples, a
//                      function of n alone, and a thread takes the groups of 4 samples g, g + 256, ... of its share: what is
//                      summed for utterance b depends on n and on its samples only, not on B, b, the padded width T or the stream.
//   warm_apply_kernel  block (tile, b): prologue — the partials of every entry folded in share order, then
//                      min_g || y - sum_s g_s e_s ||^2 by Cholesky G = L L^T; a pivot <= 2^-40 trace(G) / S (a silent estimate,
//                      two proportional ones; NaN included) sets every gain of the utterance to 1 and its fallback flag.  Every
//                      block of an utterance solves the same system from the same sums.  Then one pass, a thread = all S sources
//                      of 4 consecutive samples, plain fp32 in the order written:
//                        x0_i = ((float) g_i * e_i - mean_b) / std_b                                     normalize_batch's tgt
//                        m    = mix_norm / S  (mean_from mix)  |  (x0_0 + .. + x0_{S-1}) / S  (mean_from estimate)
//                        mu_i = m + e^{-lambda t_b} (x0_i - m)                                           MixSDE._mean
//                        x_i  = mu_i + (a mz + p (z_i - mz)) [a, p times sigma_mix],  mz = (z_0 + ..) / S  L(t_b) z
//                      with a = sqrt(ev1), p = sqrt(ev2) of mix_eig (common.h), the helper of the prior kernel.  z is the caller's
//                      or generated here: value s * n + t of the stream (seeds[b], 0) — draw 0 of diffsep_randn_batch — or, without
//                      per-utterance seeds, value (b S + s) T + t of the stream (seed, 0) — draw 0 of diffsep_randn: the draw the
//                      sampler's prior would have used.  Samples at or beyond lengths[b] are written as exact zeros.
// 16-byte accesses where every row starts on a 16-byte boundary (all bases aligned, T % 4 == 0), sample by sample otherwise; both
// paths hand the same four values to the same arithmetic.
#include <string>

#include "../../include/diffsep_hip.h"
#include "common.h"
#include "reduce_device.h"  // the fixed-order fp64 block totals

// per-sample arithmetic is plain fp32 in the order written: the float64 restatement of the tests (tests/warm_start_ref.py)
// counts its roundings operation by operation
#pragma clang fp contract(off)

namespace {

constexpr int kWarmParts = 32;  // shares (= blocks of the fit, = partial sums) per utterance
constexpr int kWarmMaxS = 3;
constexpr int kWarmNQ = kWarmMaxS * kWarmMaxS + kWarmMaxS;  // doubles per partial: G [S][S], then r [S]

__host__ __device__ inline long warm_share(long n) { return ((n + kWarmParts - 1) / kWarmParts + 3) / 4 * 4; }

__device__ inline long warm_len(const int* lens, int b, long T) {
  if (!lens) return T;
  const long n = lens[b];
  return n < 0 ? 0 : (n > T ? T : n);
}

// the four samples t .. t + 3 of a row (those at or beyond n are not read and come back as 0)
__device__ inline void warm_load4(const float* __restrict__ row, long t, long n, bool vec, float* v) {
  if (vec && t + 4 <= n) {
    const float4 q = *reinterpret_cast<const float4*>(row + t);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = t + e < n ? row[t + e] : 0.0f;
  }
}
__device__ inline void warm_store4(float* __restrict__ row, long t, long n, bool vec, const float* v) {
  if (vec && t + 4 <= n) {
    *reinterpret_cast<float4*>(row + t) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (t + e < n) row[t + e] = v[e];
  }
}

// part[b][share][kWarmNQ].  grid (kWarmParts, B), 256 threads
template <int S>
__global__ __launch_bounds__(256) void warm_fit_kernel(const float* __restrict__ est, const float* __restrict__ mix,
                                                       const int* __restrict__ lens, double* __restrict__ part, long T,
                                                       int vec) {
  constexpr int NQ = S * S + S;
  __shared__ double sh[NQ][4];
  const int p = blockIdx.x, b = blockIdx.y;
  const long n = warm_len(lens, b, T);
  const long share = warm_share(n);
  const long t0 = (long)p * share, t1 = t0 + share < n ? t0 + share : n;
  const float* e = est + (long)b * S * T;
  const float* y = mix + (long)b * T;
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  for (long t = t0 + 4 * (long)threadIdx.x; t < t1; t += 4 * 256) {
    float ev[S][4], yv[4];
    warm_load4(y, t, n, vec != 0, yv);
#pragma unroll
    for (int i = 0; i < S; ++i) warm_load4(e + (long)i * T, t, n, vec != 0, ev[i]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int i = 0; i < S; ++i) {
#pragma unroll
        for (int j = 0; j < S; ++j) acc[i * S + j] += (double)ev[i][k] * (double)ev[j][k];
        acc[S * S + i] += (double)ev[i][k] * (double)yv[k];
      }
  }
  const double r = ds_block_totals_d<4, NQ>(acc, NQ, sh);
  if ((int)threadIdx.x < NQ) part[((long)b * kWarmParts + p) * kWarmNQ + threadIdx.x] = r;
}

// G g = r by Cholesky, G [S][S] (row-major, its lower triangle is read), every operation in float64.  false: a pivot at or below
// 2^-40 trace(G) / S (or not a number) — g is then left untouched.
__device__ inline bool warm_solve(const double* G, const double* r, int S, double* g) {
  double tr = 0.0;
  for (int i = 0; i < S; ++i) tr += G[i * S + i];
  const double thr = 0x1p-40 * tr / (double)S;
  double L[kWarmMaxS][kWarmMaxS];
  for (int j = 0; j < S; ++j) {
    double d = G[j * S + j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > thr)) return false;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < S; ++i) {
      double s = G[i * S + j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  double y[kWarmMaxS];
  for (int i = 0; i < S; ++i) {  // L y = r
    double s = r[i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = S - 1; i >= 0; --i) {  // L^T g = y
    double s = y[i];
    for (int k = i + 1; k < S; ++k) s -= L[k][i] * g[k];
    g[i] = s / L[i][i];
  }
  return true;
}

struct WarmArgs {
  SdeP s;
  const float* est; const float* mixn; const float* mean; const float* std; const float* t; const float* z; const float* smix;
  const int* lens; const unsigned long long* seeds; unsigned long long seed;
  const double* part;  // null: gains of 1 (scale none)
  float* x; double* gains; int* fallback;
  int mean_from; long T; int vec;
};

// grid (ceil(ceil(T / 4) / 256), B), 256 threads
template <int S>
__global__ __launch_bounds__(256) void warm_apply_kernel(WarmArgs a) {
  constexpr int NQ = S * S + S;
  __shared__ double sums[NQ];
  __shared__ float shg[S];
  __shared__ float shc[3];  // e^{-lambda t}, sqrt(ev1), sqrt(ev2)
  const int b = blockIdx.y;
  if (a.part && (int)threadIdx.x < NQ) {
    const double* q = a.part + (long)b * kWarmParts * kWarmNQ + threadIdx.x;
    double s = q[0];
    for (int p = 1; p < kWarmParts; ++p) s += q[(long)p * kWarmNQ];
    sums[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double g[S];
    bool ok = true;
    for (int i = 0; i < S; ++i) g[i] = 1.0;
    if (a.part) {
      ok = warm_solve(sums, sums + S * S, S, g);
      if (!ok)
        for (int i = 0; i < S; ++i) g[i] = 1.0;
    }
    for (int i = 0; i < S; ++i) shg[i] = (float)g[i];
    if (blockIdx.x == 0) {
      for (int i = 0; i < S; ++i) a.gains[(long)b * S + i] = g[i];
      a.fallback[b] = ok ? 0 : 1;
    }
    const float tb = a.t[b];
    float ev1, ev2;
    mix_eig(a.s, tb, ev1, ev2);
    shc[0] = expf(-tb * a.s.d_lambda);
    shc[1] = sqrtf(ev1);
    shc[2] = sqrtf(ev2);
  }
  __syncthreads();
  const long T = a.T;
  const long t0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (t0 >= T) return;
  const long len = warm_len(a.lens, b, T);
  const bool vec = a.vec != 0;
  const float decay = shc[0], ca0 = shc[1], cp0 = shc[2];
  const float mu = a.mean[b], sd = a.std[b];
  float e[S][4], z[S][4], mn[4] = {0.f, 0.f, 0.f, 0.f}, sm[4];
  if (a.mean_from == DIFFSEP_WARM_MEAN_MIX) warm_load4(a.mixn + (long)b * T, t0, len, vec, mn);
  if (a.smix) warm_load4(a.smix + (long)b * T, t0, len, vec, sm);
  else sm[0] = sm[1] = sm[2] = sm[3] = 1.0f;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const long row = ((long)b * S + i) * T;
    warm_load4(a.est + row, t0, len, vec, e[i]);
    if (a.z) {
      warm_load4(a.z + row, t0, len, vec, z[i]);
    } else {  // 4 consecutive values of the stream lie in at most two Philox groups of four
      const unsigned long long key = a.seeds ? a.seeds[b] : a.seed;
      const uint64_t el = a.seeds ? (uint64_t)((long)i * len + t0) : (uint64_t)(row + t0);
      float v[8];
      philox_randn4(el >> 2, key, 0, v);
      if (el & 3) philox_randn4((el >> 2) + 1, key, 0, v + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) z[i][j] = v[(el & 3) + j];
    }
  }
  float xo[S][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (t0 + j >= len) {
#pragma unroll
      for (int i = 0; i < S; ++i) xo[i][j] = 0.f;
      continue;
    }
    float x0[S], m = 0.f, mz = 0.f;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      x0[i] = (shg[i] * e[i][j] - mu) / sd;
      m += x0[i];
      mz += z[i][j];
    }
    m = a.mean_from == DIFFSEP_WARM_MEAN_MIX ? mn[j] / (float)S : m / (float)S;
    mz /= (float)S;
    const float ca = ca0 * sm[j], cp = cp0 * sm[j];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const float mean = m + decay * (x0[i] - m);
      const float lz = ca * mz + cp * (z[i][j] - mz);
      xo[i][j] = mean + lz;
    }
  }
  // (rows are written over the whole width T: zeros from len on)
#pragma unroll
  for (int i = 0; i < S; ++i) warm_store4(a.x + ((long)b * S + i) * T, t0, T, vec, xo[i]);
}

int64_t warm_workspace(int B) { return ((int64_t)B * kWarmParts * kWarmNQ * 8 + 255) / 256 * 256; }

std::string warm_bad_shape(int64_t B, int64_t S, int64_t T) {
  if (S < 1 || S > kWarmMaxS) return "S = " + std::to_string(S) + " sources (1..3)";
  if (B < 1 || B > 65535) return "B = " + std::to_string(B) + " utterances (1..65535)";
  if (T < 1 || T >= ((int64_t)1 << 31)) return "T = " + std::to_string(T) + " samples (1 .. 2^31 - 1)";
  return "";
}

}  // namespace

extern "C" int64_t diffsep_warm_start_workspace_bytes(int32_t B, int32_t S) {
  const std::string why = warm_bad_shape(B, S, 1);
  if (!why.empty()) {
    ds_set_error("warm_start_workspace_bytes: " + why);
    return -1;
  }
  return warm_workspace(B);
}

extern "C" int32_t diffsep_warm_start(const diffsep_sde_config* sde, const float* est, const float* mix, const float* mix_norm,
                                      const float* mean, const float* std, const float* t, const float* z,
                                      const float* sigma_mix, const int32_t* lengths, const uint64_t* seeds, uint64_t seed,
                                      int32_t scale, int32_t mean_from, float* x_init, double* gains_out, int32_t* fallback_out,
                                      int32_t B, int32_t S, int64_t T, void* workspace, int64_t workspace_bytes, void* stream) {
  const std::string why = warm_bad_shape(B, S, T);
  DS_CHECK(why.empty(), "warm_start: " + why);
  DS_CHECK(sde && est && mean && std && t && x_init && gains_out && fallback_out, "warm_start: null argument");
  DS_CHECK(sde->kind == DIFFSEP_SDE_MIX || sde->kind == DIFFSEP_SDE_PRIORMIX, "warm_start: unknown SDE kind");
  DS_CHECK((sde->kind == DIFFSEP_SDE_PRIORMIX) == (sigma_mix != nullptr),
           "warm_start: PriorMixSDE needs sigma_mix, MixSDE must not get one");
  DS_CHECK(scale == DIFFSEP_WARM_SCALE_NONE || scale == DIFFSEP_WARM_SCALE_LS, "warm_start: scale must be none (0) or ls (1)");
  DS_CHECK(mean_from == DIFFSEP_WARM_MEAN_MIX || mean_from == DIFFSEP_WARM_MEAN_ESTIMATE,
           "warm_start: mean_from must be mix (0) or estimate (1)");
  DS_CHECK(mean_from != DIFFSEP_WARM_MEAN_MIX || mix_norm, "warm_start: mean_from = mix needs mix_norm");
  DS_CHECK(!(z && seeds), "warm_start: per-utterance seeds are for generated noise (z == NULL)");
  const bool fit = scale == DIFFSEP_WARM_SCALE_LS;
  if (fit) {
    DS_CHECK(mix, "warm_start: scale = ls needs the raw mixture");
    DS_CHECK(workspace, "warm_start: scale = ls needs a workspace");
    DS_CHECK(workspace_bytes >= warm_workspace(B), "warm_start: workspace too small (workspace_bytes = " +
                                                       std::to_string(workspace_bytes) + " < " +
                                                       std::to_string(warm_workspace(B)) + ")");
    DS_CHECK(((uintptr_t)workspace & 7) == 0, "warm_start: workspace must be 8-byte aligned");
  }
  hipStream_t st = (hipStream_t)stream;
  const uintptr_t bases = (uintptr_t)est | (uintptr_t)mix | (uintptr_t)mix_norm | (uintptr_t)z | (uintptr_t)sigma_mix | (uintptr_t)x_init;
  const int vec = (bases & 15) == 0 && T % 4 == 0;
  double* part = fit ? (double*)workspace : nullptr;
  if (fit) {
    const dim3 gf(kWarmParts, B);
    if (S == 1) warm_fit_kernel<1><<<gf, 256, 0, st>>>(est, mix, lengths, part, T, vec);
    else if (S == 2) warm_fit_kernel<2><<<gf, 256, 0, st>>>(est, mix, lengths, part, T, vec);
    else warm_fit_kernel<3><<<gf, 256, 0, st>>>(est, mix, lengths, part, T, vec);
    DS_LAUNCH_CHECK();
  }
  WarmArgs a;
  a.s.kind = sde->kind; a.s.ndim = sde->ndim; a.s.d_lambda = sde->d_lambda; a.s.sigma_min = sde->sigma_min; a.s.sigma_max = sde->sigma_max;
  a.est = est; a.mixn = mix_norm; a.mean = mean; a.std = std; a.t = t; a.z = z; a.smix = sigma_mix;
  a.lens = lengths; a.seeds = (const unsigned long long*)seeds; a.seed = seed; a.part = part;
  a.x = x_init; a.gains = gains_out; a.fallback = fallback_out; a.mean_from = mean_from; a.T = T; a.vec = vec;
  const dim3 ga((unsigned)(((T + 3) / 4 + 255) / 256), B);
  if (S == 1) warm_apply_kernel<1><<<ga, 256, 0, st>>>(a);
  else if (S == 2) warm_apply_kernel<2><<<ga, 256, 0, st>>>(a);
  else warm_apply_kernel<3><<<ga, 256, 0, st>>>(a);
  DS_LAUNCH_CHECK();
  return 0;
}
