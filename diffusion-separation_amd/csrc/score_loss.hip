// score_loss.hip — the denoising score-matching loss of the reference's DiffSepModel (pl_model.py:179-247 sample_prior,
// :327-424 the loss forms) as two HBM-bound streaming passes over [B,S,T] fp32 waveforms around one score evaluation:
//   perturb      x_t = beta true_mix + (1 - beta) mean + L z,  z' = z + beta L^-1 (true_mix - mean)   (every init_hack mode)
//   loss_reduce  out[b][p] = mean_{s, t < len_b} ((L score)[s,t] + z_p[s,t])^2,  z_p = z + L^-1 (anchor - mean_p)
// with  mean = (A + e^{-lambda t} Pn) x0,  L = (sqrt(ev1) A + sqrt(ev2) Pn) [sigma_mix]  (sdes/sdes.py:286-320, 515-532).
// A and Pn are complementary projectors, so L^-1 = (A / sqrt(ev1) + Pn / sqrt(ev2)) [/ sigma_mix]: no linear solve.  The source
// permutations of the PIT losses all see the same x_t (pl_model.py:343, 391 with z = z0 + L^-1 (true_mix - mean)), so one
// score evaluation and one reduction pass with S! accumulators replace the reference's S! network evaluations.
// One thread owns all S sources of 4 consecutive samples, whatever the alignment (128-bit accesses when T % 4 == 0 and the
// pointers allow, scalar otherwise): the order of every sum depends on the sample index alone.
#include "engine_host.h"
#include "reduce_device.h"  // the fixed-order fp64 block totals of the loss partials and the finishing pass

// per-sample arithmetic is plain fp32 in the order written: the float64 restatement of the tests (tests/score_loss_cases.py)
// follows it operation by operation, which a fused multiply-add here and not there would break
#pragma clang fp contract(off)

#define SL_MAX_SRC 3  // S! accumulators: 6 for S = 3 (arch.hip: num_sources is 1..3)
#define SL_MAX_P 6
// itertools.permutations(range(S)) (pl_model.py:347, 383)
__constant__ int c_perm3[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

struct SlCoef { float decay, a, p; };  // e^{-lambda t}, sqrt(ev1), sqrt(ev2): once per block
__device__ inline SlCoef sl_coef(const SdeP& s, float t) {
  float ev1, ev2;
  mix_eig(s, t, ev1, ev2);
  SlCoef c;
  c.decay = expf(-t * s.d_lambda);
  c.a = sqrtf(ev1);
  c.p = sqrtf(ev2);
  return c;
}
// 4 consecutive samples of a row (zero beyond T in the scalar form)
template <bool VEC>
__device__ inline void sl_ld4(const float* row, long t0, long T, float* v) {
  if (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(row + t0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (t0 + j < T) ? row[t0 + j] : 0.f;
  }
}
template <bool VEC>
__device__ inline void sl_st4(float* row, long t0, long T, const float* v) {
  if (VEC) {
    *reinterpret_cast<float4*>(row + t0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t0 + j < T) row[t0 + j] = v[j];
  }
}
// L^-1 d = A d / a + Pn d / p  at one sample (d [S] -> e [S])
template <int S>
__device__ inline void sl_linv(const float* d, float a, float p, float* e) {
  float md = 0.f;
#pragma unroll
  for (int i = 0; i < S; ++i) md += d[i];
  md /= (float)S;
#pragma unroll
  for (int i = 0; i < S; ++i) e[i] = md / a + (d[i] - md) / p;
}

struct PerturbArgs {
  SdeP s;
  const float* x0; const float* mix; const float* t; const float* z; const float* smix; const float* beta;
  const int* lens;
  float* xt; float* zo;
  uint64_t seed, sid;
  int redefine; long T;
};

// (z and zo may be the same buffer: a thread reads its own samples before it writes them)
template <int S, bool VEC>
__global__ __launch_bounds__(256) void sde_perturb_kernel(PerturbArgs a) {
  __shared__ SlCoef shc;
  const int b = blockIdx.y;
  if (threadIdx.x == 0) shc = sl_coef(a.s, a.t[b]);
  __syncthreads();
  const long t0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  const long T = a.T;
  if (t0 >= T) return;
  const SlCoef c = shc;
  const float beta = a.beta ? a.beta[b] : 0.f;
  const long len = a.lens ? min((long)a.lens[b], T) : T;
  float x[S][4], z[S][4], m[4], sm[4];
  sl_ld4<VEC>(a.mix + (long)b * T, t0, T, m);
  if (a.smix) sl_ld4<VEC>(a.smix + (long)b * T, t0, T, sm);
  else sm[0] = sm[1] = sm[2] = sm[3] = 1.0f;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const long row = ((long)b * S + i) * T;
    sl_ld4<VEC>(a.x0 + row, t0, T, x[i]);
    if (a.z) {
      sl_ld4<VEC>(a.z + row, t0, T, z[i]);
    } else if (VEC) {  // T % 4 == 0: element row + t0 opens a Philox group of four
      philox_randn4((uint64_t)(row + t0) >> 2, a.seed, a.sid, z[i]);
    } else {  // 4 consecutive elements lie in at most two Philox groups of four
      const uint64_t el = (uint64_t)(row + t0);
      float v[8];
      philox_randn4(el >> 2, a.seed, a.sid, v);
      if (el & 3) philox_randn4((el >> 2) + 1, a.seed, a.sid, v + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) z[i][j] = v[(el & 3) + j];
    }
  }
  float xo[S][4], zo[S][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (t0 + j >= len) {
#pragma unroll
      for (int i = 0; i < S; ++i) { xo[i][j] = 0.f; zo[i][j] = 0.f; }
      continue;
    }
    const float ca = c.a * sm[j], cp = c.p * sm[j];
    const float tm = m[j] / (float)S;  // true_mix = mix / S   pl_model.py:191
    float mx = 0.f, mz = 0.f;
#pragma unroll
    for (int i = 0; i < S; ++i) { mx += x[i][j]; mz += z[i][j]; }
    mx /= (float)S;
    mz /= (float)S;
    float d[S], e[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const float mean = mx + c.decay * (x[i][j] - mx);
      const float lz = ca * mz + cp * (z[i][j] - mz);
      xo[i][j] = (tm * beta + mean * (1.0f - beta)) + lz;  // pl_model.py:211 (beta = 0: mean + L z, :245)
      d[i] = tm - mean;
    }
    if (a.redefine && beta != 0.f) {
      sl_linv<S>(d, ca, cp, e);
#pragma unroll
      for (int i = 0; i < S; ++i) zo[i][j] = z[i][j] + beta * e[i];
    } else {
#pragma unroll
      for (int i = 0; i < S; ++i) zo[i][j] = z[i][j];
    }
  }
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const long row = ((long)b * S + i) * T;
    sl_st4<VEC>(a.xt + row, t0, T, xo[i]);
    sl_st4<VEC>(a.zo + row, t0, T, zo[i]);
  }
}

struct LossArgs {
  SdeP s;
  const float* score; const float* z; const float* x0; const float* mix; const float* t; const float* smix;
  const int* lens;
  double* part;  // [B][nblk][SL_MAX_P]
  float* coef_out;
  int P, mode; long T;
};

template <int S, bool VEC>
__global__ __launch_bounds__(256) void score_loss_partial_kernel(LossArgs a) {
  __shared__ SlCoef shc;
  __shared__ double sh[SL_MAX_P][4];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    shc = sl_coef(a.s, a.t[b]);
    if (a.coef_out && blockIdx.x == 0) {
      a.coef_out[3 * b] = shc.decay; a.coef_out[3 * b + 1] = shc.a; a.coef_out[3 * b + 2] = shc.p;
    }
  }
  __syncthreads();
  const SlCoef c = shc;
  const long T = a.T;
  const long len = a.lens ? min((long)a.lens[b], T) : T;
  const long t0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  double acc[SL_MAX_P];
#pragma unroll
  for (int p = 0; p < SL_MAX_P; ++p) acc[p] = 0.0;
  if (t0 < len) {
    float g[S][4], z[S][4], x[S][4], m[4], sm[4];
    if (a.smix) sl_ld4<VEC>(a.smix + (long)b * T, t0, T, sm);
    else sm[0] = sm[1] = sm[2] = sm[3] = 1.0f;
    const bool pit = a.mode != 0;
    if (pit) sl_ld4<VEC>(a.mix + (long)b * T, t0, T, m);
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const long row = ((long)b * S + i) * T;
      sl_ld4<VEC>(a.score + row, t0, T, g[i]);
      sl_ld4<VEC>(a.z + row, t0, T, z[i]);
      if (pit) sl_ld4<VEC>(a.x0 + row, t0, T, x[i]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (t0 + j >= len) continue;
      const float ca = c.a * sm[j], cp = c.p * sm[j];
      float mg = 0.f;
#pragma unroll
      for (int i = 0; i < S; ++i) mg += g[i][j];
      mg /= (float)S;
      float ls[S];
#pragma unroll
      for (int i = 0; i < S; ++i) ls[i] = ca * mg + cp * (g[i][j] - mg);  // mult_std(L, pred_score)
      if (!pit) {
#pragma unroll
        for (int i = 0; i < S; ++i) {
          const double r = (double)(ls[i] + z[i][j]);  // loss(L_score, -z): pl_model.py:418-419
          acc[0] += r * r;
        }
        continue;
      }
      const float tm = m[j] / (float)S;
      float mx = 0.f;
#pragma unroll
      for (int i = 0; i < S; ++i) mx += x[i][j];
      mx /= (float)S;
      float mean0[S];
#pragma unroll
      for (int i = 0; i < S; ++i) mean0[i] = mx + c.decay * (x[i][j] - mx);
#pragma unroll
      for (int p = 0; p < SL_MAX_P; ++p) {
        if (p >= a.P) break;
        float d[S], e[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
          // source i of permutation p (S = 2: identity, swap; S = 3: the table; S = 1: itself)
          const int src = S == 3 ? c_perm3[p][i] : (S == 2 ? (p == 0 ? i : 1 - i) : 0);
          float mp = mean0[0];
#pragma unroll
          for (int k = 1; k < S; ++k) mp = (src == k) ? mean0[k] : mp;
          d[i] = (a.mode == 1 ? tm : mean0[i]) - mp;  // pl_model.py:387 (true_mix - mean) / :352 (mean_0 - mean_p)
        }
        sl_linv<S>(d, ca, cp, e);
#pragma unroll
        for (int i = 0; i < S; ++i) {
          const float zp = z[i][j] + e[i];
          const double r = (double)(ls[i] + zp);
          acc[p] += r * r;
        }
      }
    }
  }
  // per-block partials in the fixed order of reduce_device.h (no float atomics)
  const double r = ds_block_totals_d<4, SL_MAX_P>(acc, a.P, sh);
  if ((int)threadIdx.x < a.P) a.part[((long)b * gridDim.x + blockIdx.x) * SL_MAX_P + threadIdx.x] = r;
}

// one finishing block per utterance: partials in a fixed order, the mean, the best permutation (first minimum)
__global__ __launch_bounds__(256) void score_loss_final_kernel(const double* __restrict__ part, int nblk, int P, int S,
                                                               long T, const int* __restrict__ lens,
                                                               double* __restrict__ out, double* __restrict__ best,
                                                               int* __restrict__ argbest) {
  __shared__ double sh[SL_MAX_P][4];
  __shared__ double tot[SL_MAX_P];
  const int b = blockIdx.x;
  double r[SL_MAX_P] = {};
#pragma unroll
  for (int p = 0; p < SL_MAX_P; ++p) {
    if (p >= P) break;
    for (int i = threadIdx.x; i < nblk; i += 256) r[p] = r[p] + part[((long)b * nblk + i) * SL_MAX_P + p];
  }
  double s = ds_block_totals_d<4, SL_MAX_P>(r, P, sh);
  if ((int)threadIdx.x < P) {
    const long len = lens ? max(0L, min((long)lens[b], T)) : T;  // (as the partial pass clamps; an empty row scores 0)
    s = len > 0 ? s / ((double)S * (double)len) : 0.0;
    tot[threadIdx.x] = s;
    out[(long)b * P + threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0 && (best || argbest)) {
    int k = 0;
    for (int p = 1; p < P; ++p)
      if (tot[p] < tot[k]) k = p;
    if (best) best[b] = tot[k];
    if (argbest) argbest[b] = k;
  }
}

// out = std^-1 x for a dense std: MixSDE.mult_std_inv (torch.linalg.solve, sdes/sdes.py:330-332) /
// PriorMixSDE.mult_std_inv (:534-558: the explicit 2x2 formula for S = 2, a solve per sample otherwise)
__global__ __launch_bounds__(256) void sde_mult_std_inv_kernel(const float* __restrict__ L, const float* __restrict__ x,
                                                               float* __restrict__ out, int S, long T, int per_t) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= T) return;
  if (S == 2 && per_t) {
    const long l0 = (long)b * 4;
    const float A = L[(l0 + 0) * T + t], Bq = L[(l0 + 1) * T + t], Cq = L[(l0 + 2) * T + t], D = L[(l0 + 3) * T + t];
    const float x1 = x[((long)b * 2) * T + t], x2 = x[((long)b * 2 + 1) * T + t];
    const float div = 1.0f / (A * D - Cq * Bq);
    out[((long)b * 2) * T + t] = div * (D * x1 - Bq * x2);
    out[((long)b * 2 + 1) * T + t] = div * (A * x2 - Cq * x1);
    return;
  }
  // LU with partial pivoting on a DS_MAX_SRC x DS_MAX_SRC system padded with the identity: every loop is unrolled and
  // every index is a constant, so the matrix stays in registers
  float M[DS_MAX_SRC][DS_MAX_SRC], v[DS_MAX_SRC];
#pragma unroll
  for (int r = 0; r < DS_MAX_SRC; ++r) {
#pragma unroll
    for (int cc = 0; cc < DS_MAX_SRC; ++cc) {
      float e = (r == cc) ? 1.0f : 0.0f;
      if (r < S && cc < S) {
        const long li = ((long)b * S + r) * S + cc;
        e = per_t ? L[li * T + t] : L[li];
      }
      M[r][cc] = e;
    }
    v[r] = r < S ? x[((long)b * S + r) * T + t] : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < DS_MAX_SRC; ++k) {
#pragma unroll
    for (int r = k + 1; r < DS_MAX_SRC; ++r) {  // bring the largest |M[r][k]|, r >= k, into row k
      const bool sw = fabsf(M[r][k]) > fabsf(M[k][k]);
#pragma unroll
      for (int cc = 0; cc < DS_MAX_SRC; ++cc) {
        const float u = M[k][cc], q = M[r][cc];
        M[k][cc] = sw ? q : u;
        M[r][cc] = sw ? u : q;
      }
      const float u = v[k], q = v[r];
      v[k] = sw ? q : u;
      v[r] = sw ? u : q;
    }
#pragma unroll
    for (int r = k + 1; r < DS_MAX_SRC; ++r) {
      const float f = M[r][k] / M[k][k];
#pragma unroll
      for (int cc = k + 1; cc < DS_MAX_SRC; ++cc) M[r][cc] = M[r][cc] - f * M[k][cc];
      v[r] = v[r] - f * v[k];
    }
  }
#pragma unroll
  for (int r = DS_MAX_SRC - 1; r >= 0; --r) {
    float acc = v[r];
#pragma unroll
    for (int cc = r + 1; cc < DS_MAX_SRC; ++cc) acc = acc - M[r][cc] * v[cc];
    v[r] = acc / M[r][r];
  }
#pragma unroll
  for (int r = 0; r < DS_MAX_SRC; ++r)
    if (r < S) out[((long)b * S + r) * T + t] = v[r];
}

// ------------------------------------------------------------------ launchers
static bool sl_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static long sl_nblk(long T) { return ((T + 3) / 4 + 255) / 256; }
static int sl_fact(int S) { return S == 3 ? 6 : (S == 2 ? 2 : 1); }
static size_t sl_slab_bytes(int B, long T) { return (size_t)B * sl_nblk(T) * SL_MAX_P * sizeof(double); }

static int check_shape(const char* who, const SdeP& s, int B, int S, long T, bool has_smix) {
  const std::string w(who);
  DS_CHECK(S >= 1 && S <= SL_MAX_SRC, w + ": the number of sources must be 1..3");
  DS_CHECK(B >= 1 && T >= 1, w + ": empty batch or signal");
  DS_CHECK(s.kind == DIFFSEP_SDE_MIX || s.kind == DIFFSEP_SDE_PRIORMIX, w + ": unknown SDE kind");
  DS_CHECK((s.kind == DIFFSEP_SDE_PRIORMIX) == has_smix, w + ": PriorMixSDE needs sigma_mix, MixSDE must not get one");
  return 0;
}

static int launch_perturb(const PerturbArgs& a, int B, int S, hipStream_t st) {
  bool vec = a.T % 4 == 0;
  const void* ps[] = {a.x0, a.mix, a.z, a.smix, a.xt, a.zo};
  for (const void* p : ps) vec = vec && sl_al16(p);
  const dim3 grid((unsigned)sl_nblk(a.T), B), blk(256);
#define SL_PERTURB(SS)                                                                      \
  if (vec) hipLaunchKernelGGL((sde_perturb_kernel<SS, true>), grid, blk, 0, st, a);         \
  else hipLaunchKernelGGL((sde_perturb_kernel<SS, false>), grid, blk, 0, st, a)
  if (S == 1) { SL_PERTURB(1); } else if (S == 2) { SL_PERTURB(2); } else { SL_PERTURB(3); }
#undef SL_PERTURB
  DS_LAUNCH_CHECK();
  return 0;
}

static int launch_reduce(LossArgs a, int B, int S, const int* lens, double* out, double* best, int* argbest,
                         hipStream_t st) {
  bool vec = a.T % 4 == 0;
  const void* ps[] = {a.score, a.z, a.x0, a.mix, a.smix};
  for (const void* p : ps) vec = vec && sl_al16(p);
  const int nblk = (int)sl_nblk(a.T);
  const dim3 grid(nblk, B), blk(256);
#define SL_REDUCE(SS)                                                                           \
  if (vec) hipLaunchKernelGGL((score_loss_partial_kernel<SS, true>), grid, blk, 0, st, a);      \
  else hipLaunchKernelGGL((score_loss_partial_kernel<SS, false>), grid, blk, 0, st, a)
  if (S == 1) { SL_REDUCE(1); } else if (S == 2) { SL_REDUCE(2); } else { SL_REDUCE(3); }
#undef SL_REDUCE
  DS_LAUNCH_CHECK();
  hipLaunchKernelGGL(score_loss_final_kernel, dim3(B), blk, 0, st, a.part, nblk, a.P, S, a.T, lens, out, best, argbest);
  DS_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ C-ABI
extern "C" int32_t diffsep_sde_mult_std_inv(const float* std, const float* x, float* out, int32_t B, int32_t S, int64_t T,
                                            int32_t per_sample, void* stream) {
  DS_CHECK(std && x && out, "sde_mult_std_inv: null pointer");
  DS_CHECK(S >= 1 && S <= DS_MAX_SRC, "sde_mult_std_inv: too many sources");
  DS_CHECK(B >= 1 && T >= 1, "sde_mult_std_inv: empty batch or signal");
  hipLaunchKernelGGL(sde_mult_std_inv_kernel, dim3(cdiv(T, 256), B), dim3(256), 0, (hipStream_t)stream, std, x, out, S,
                     (long)T, per_sample);
  DS_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t diffsep_sde_perturb(const diffsep_sde_config* sde, const float* x0, const float* mix, const float* t,
                                       const float* z, const float* sigma_mix, const float* beta, int32_t redefine_z,
                                       const int32_t* lengths, uint64_t seed, uint64_t stream_id, float* x_t,
                                       float* z_out, int32_t B, int32_t S, int64_t T, void* stream) {
  DS_CHECK(sde && x0 && mix && t && x_t && z_out, "sde_perturb: null pointer");
  PerturbArgs a;
  a.s = to_sdep(sde);
  if (check_shape("sde_perturb", a.s, B, S, T, sigma_mix != nullptr)) return 1;
  a.x0 = x0; a.mix = mix; a.t = t; a.z = z; a.smix = sigma_mix; a.beta = beta; a.lens = lengths;
  a.xt = x_t; a.zo = z_out; a.seed = seed; a.sid = stream_id; a.redefine = redefine_z; a.T = T;
  return launch_perturb(a, B, S, (hipStream_t)stream);
}

extern "C" int64_t diffsep_score_loss_workspace_bytes(int32_t B, int32_t S, int64_t T) {
  if (!(B >= 1 && S >= 1 && S <= SL_MAX_SRC && T >= 1)) {
    ds_set_error("score_loss_workspace_bytes: B >= 1, S in 1..3 and T >= 1 expected");
    return -1;
  }
  return (int64_t)sl_slab_bytes(B, T);
}

extern "C" int32_t diffsep_score_loss_reduce(const diffsep_sde_config* sde, const float* score, const float* z,
                                             const float* x0, const float* mix, const float* t,
                                             const float* sigma_mix, const int32_t* lengths, int32_t pit_mode,
                                             double* out, double* best, int32_t* argbest, float* coef_out, int32_t B,
                                             int32_t S, int64_t T, void* workspace, int64_t workspace_bytes,
                                             void* stream) {
  DS_CHECK(sde && score && z && t && out && workspace, "score_loss_reduce: null pointer");
  LossArgs a;
  a.s = to_sdep(sde);
  if (check_shape("score_loss_reduce", a.s, B, S, T, sigma_mix != nullptr)) return 1;
  DS_CHECK(pit_mode >= 0 && pit_mode <= 2, "score_loss_reduce: pit_mode must be 0 (none), 1 (true-mix anchor) or 2 (mean_0 anchor)");
  DS_CHECK(pit_mode == 0 || (x0 && mix), "score_loss_reduce: the PIT forms need x0 and mix");
  DS_CHECK(workspace_bytes >= (int64_t)sl_slab_bytes(B, T),
           "score_loss_reduce: workspace too small (diffsep_score_loss_workspace_bytes)");
  a.score = score; a.z = z; a.x0 = x0; a.mix = mix; a.t = t; a.smix = sigma_mix; a.lens = lengths;
  a.part = (double*)workspace; a.coef_out = coef_out; a.P = pit_mode ? sl_fact(S) : 1; a.mode = pit_mode; a.T = T;
  return launch_reduce(a, B, S, lengths, out, best, argbest, (hipStream_t)stream);
}

extern "C" int32_t diffsep_score_loss_validate(const diffsep_model_config* cfg, const diffsep_loss_config* loss, int32_t B,
                                               int64_t T, const int64_t* lengths_host, int64_t workspace_bytes) {
  DS_CHECK(cfg && loss, "score_loss: null argument");
  DS_CHECK(cfg->num_sources >= 1 && cfg->num_sources <= SL_MAX_SRC, "score_loss: the number of sources must be 1..3");
  DS_CHECK(B >= 1 && T >= 1, "score_loss: empty batch or signal");
  DS_CHECK(loss->pit_mode >= 0 && loss->pit_mode <= 2,
           "score_loss: pit_mode must be 0 (none), 1 (true-mix anchor) or 2 (mean_0 anchor)");
  if (check_batch_ext(cfg, "score_loss", B, T, lengths_host, nullptr, nullptr, nullptr, nullptr)) return 1;
  DS_CHECK(workspace_bytes >= (int64_t)sl_slab_bytes(B, T),
           "score_loss: workspace too small (diffsep_score_loss_workspace_bytes)");
  return 0;
}

extern "C" int32_t diffsep_score_loss(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_loss_config* cfg,
                                      const float* mix_norm, const float* target, const float* t, const float* beta,
                                      const float* z, uint64_t seed, const int64_t* lengths_host, double* out,
                                      double* best, int32_t* argbest, float* x_t_out, float* score_out, int32_t B,
                                      int64_t T, void* workspace, int64_t workspace_bytes, void* stream) {
  DS_CHECK(e && sde && cfg && mix_norm && target && t && out && workspace, "score_loss: null argument");
  if (diffsep_score_loss_validate(&e->cfg, cfg, B, T, lengths_host, workspace_bytes)) return 1;
  if (check_sde(e, sde, "score_loss")) return 1;
  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  const int S = e->cfg.num_sources;
  if (ensure_plan(e, B, T, st)) return 1;
  const size_t nst = (size_t)B * S * T;
  // the resident state of the sampler serves: st_mix, st_t, st_x = x_t, st_noise = z', st_score
  DS_HIP(hipMemcpyAsync(e->st_mix, mix_norm, (size_t)B * T * 4, hipMemcpyDeviceToDevice, st));
  DS_HIP(hipMemcpyAsync(e->st_t, t, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  const int* lens = nullptr;
  if (lengths_host) {  // -> device through pinned staging, stream-ordered
    char* raw;
    if (e->ext_pin.acquire((size_t)B * 16, &raw)) return 1;
    int* pin = reinterpret_cast<int*>(raw);
    for (int b = 0; b < B; ++b) pin[b] = (int)lengths_host[b];
    DS_HIP(hipMemcpyAsync(e->st_lens, pin, (size_t)B * 4, hipMemcpyHostToDevice, st));
    if (e->ext_pin.record(st)) return 1;
    lens = e->st_lens;
    if (ds_launch_mask_tail(e->st_mix, B, 1, T, lens, st)) return 1;
  }
  const float* smix = nullptr;
  if (mixture_scale(e, sde, B, T, st, &smix)) return 1;
  PerturbArgs pa;
  pa.s = to_sdep(sde);
  pa.x0 = target; pa.mix = e->st_mix; pa.t = e->st_t; pa.z = z; pa.smix = smix; pa.beta = beta; pa.lens = lens;
  pa.xt = e->st_x; pa.zo = e->st_noise; pa.seed = seed; pa.sid = 0; pa.redefine = cfg->redefine_z; pa.T = T;
  // algorithmic bytes: x0, mix (and z, sigma_mix) read once, x_t and z' written once
  const double pb = 4.0 * ((double)nst * (z ? 4.0 : 3.0) + (double)B * T * (smix ? 2.0 : 1.0));
  if (prof_launch(e, st, hbm_rec("sde_perturb (sample_prior)", pb, B, 1, (int)T, S), [&]() { return launch_perturb(pa, B, S, st); }))
    return 1;
  if (run_nfe(e, B, T, st)) return 1;
  LossArgs la;
  la.s = pa.s;
  la.score = e->st_score; la.z = e->st_noise; la.x0 = target; la.mix = e->st_mix; la.t = e->st_t; la.smix = smix;
  la.lens = lens; la.part = (double*)workspace; la.coef_out = nullptr;
  la.P = cfg->pit_mode ? sl_fact(S) : 1; la.mode = cfg->pit_mode; la.T = T;
  const double rb = 4.0 * ((double)nst * (cfg->pit_mode ? 3.0 : 2.0) + (double)B * T * ((smix ? 1.0 : 0.0) + (cfg->pit_mode ? 1.0 : 0.0)));
  if (prof_launch(e, st, hbm_rec("score_loss_reduce", rb, B, 1, (int)T, S),
                  [&]() { return launch_reduce(la, B, S, lens, out, best, argbest, st); }))
    return 1;
  if (x_t_out) DS_HIP(hipMemcpyAsync(x_t_out, e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
  if (score_out) DS_HIP(hipMemcpyAsync(score_out, e->st_score, nst * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}
