// longform.hip — long recordings: a file of T samples as K windows of Tw samples, and the windows put back together on the device.
//
// The plan (host arithmetic, diffsep_longform_plan): T <= Tw is one window, the file itself.  Otherwise hop = Tw - Tv,
// K = 1 + ceil((T - Tw) / hop), starts[k] = k hop for k < K - 1 and starts[K - 1] = T - Tw (the last window is shifted back to
// end at T: every window is full length).  Windows k and k + 1 overlap on [starts[k + 1], starts[k] + Tw), at least Tv samples
// and more only for the last pair; their seam is the n = min(Tv, overlap) samples at the centre of the overlap.  With
// 3 Tv <= Tw seams never intersect and every sample outside them lies in exactly one window's own stretch (lf_locate).
//
// A separator emits its sources in an arbitrary order per window, so the stitch aligns before it cross-fades.  Three launches,
// asynchronous, no readback; the kernels recompute the plan from (T, Tw, Tv, K), no table is uploaded:
//   lf_gram_kernel   per pair k and block: partial sums of C_k[i][j] = sum over the overlap of win[k][i] win[k + 1][j]; every
//                    product of two floats is exact in float64, the sums are float64 in the fixed order of reduce_device.h
//   lf_perm_kernel   one block: finishes the sums (block partials in order), then one thread walks the pairs: r_k = the
//                    permutation of largest sum_i C_k[i][r(i)] (lexicographic order, strict >: a tie keeps the earliest, the
//                    identity among them), g_0 = identity, g_{k+1}[i] = r_k[g_k[i]]; perm_out[k] = g_k
//   lf_blend_kernel  one thread per output sample: the owning window's row g_k[i], or inside a seam a + (b - a) r with
//                    r = (j + 0.5) / n in float32, unfused: where both windows agree the result is that value bit for bit
#include <string>

#include "../../include/diffsep_hip.h"
#include "common.h"
#include "perm_search.h"    // the permutation rule (lexicographic candidates, strict >), shared with ensemble.hip
#include "reduce_device.h"  // the fixed-order fp64 block totals of the cross-Gram partials

namespace {

constexpr int kLfBlocks = 16;  // blocks (= partial sums) per pair of the cross-Gram: K = 17 windows fill 256 compute units once
constexpr int kLfMaxS = 3;

struct LfPlan { long T, Tw, Tv, hop; int K; };

// "" and the plan, or why the request is refused
std::string lf_make_plan(int64_t T, int64_t Tw, int64_t Tv, LfPlan* p) {
  if (T < 1) return "T = " + std::to_string(T) + " < 1";
  if (Tv < 1) return "overlap Tv = " + std::to_string(Tv) + " < 1";
  if (Tw < 1 || Tv > Tw / 3) return "3 Tv > Tw (Tv = " + std::to_string(Tv) + ", Tw = " + std::to_string(Tw) + "): seams would intersect";
  if (T > ((int64_t)1 << 46) || Tw > ((int64_t)1 << 46)) return "T or Tw beyond 2^46";
  p->T = T; p->Tw = Tw; p->Tv = Tv; p->hop = Tw - Tv;
  int64_t K = 1;
  if (T > Tw) K = 1 + (T - Tw + p->hop - 1) / p->hop;
  if (K > ((int64_t)1 << 24)) return "more than 2^24 windows";
  p->K = (int)K;
  return "";
}

__host__ __device__ inline long lf_start(const LfPlan& p, int k) {
  return p.K == 1 ? 0 : (k < p.K - 1 ? (long)k * p.hop : p.T - p.Tw);
}
__host__ __device__ inline long lf_overlap(const LfPlan& p, int k) { return lf_start(p, k) + p.Tw - lf_start(p, k + 1); }

// Where sample t of the file comes from: window *k alone (*n = 0), or the seam of pair (*k, *k + 1) at offset *j of *n.
__host__ __device__ inline void lf_locate(const LfPlan& p, long t, int* k, long* j, long* n) {
  *j = 0; *n = 0;
  if (p.K == 1) { *k = 0; return; }
  const long ovl = lf_overlap(p, p.K - 2), nl = ovl < p.Tv ? ovl : p.Tv;  // the last pair: the only overlap that may be longer
  const long sl = lf_start(p, p.K - 1) + (ovl - nl) / 2;
  if (t >= sl + nl) { *k = p.K - 1; return; }
  if (t >= sl) { *k = p.K - 2; *j = t - sl; *n = nl; return; }
  long q = t / p.hop;  // t < sl: the seams before the last one are [m hop, m hop + Tv), m = 1 .. K - 2
  if (q > p.K - 2) q = p.K - 2;
  const long off = t - q * p.hop;
  if (q >= 1 && off < p.Tv) { *k = (int)q - 1; *j = off; *n = p.Tv; return; }
  *k = (int)q;
}

// part[pair][blk][S][S]: block blk of pair sums its contiguous share of the overlap, thread t the samples t, t + 256, ... of it,
// then the block totals in the fixed order of reduce_device.h.  grid ((K - 1) kLfBlocks), 256 threads
template <int S>
__global__ __launch_bounds__(256) void lf_gram_kernel(const float* __restrict__ win, double* __restrict__ part, LfPlan p) {
  __shared__ double sh[S * S][4];
  const int pair = blockIdx.x / kLfBlocks, blk = blockIdx.x % kLfBlocks;
  const long ov = lf_overlap(p, pair);
  const long share = (ov + kLfBlocks - 1) / kLfBlocks;
  const long j0 = (long)blk * share, j1 = j0 + share < ov ? j0 + share : ov;
  const long oa = lf_start(p, pair + 1) - lf_start(p, pair);  // the overlap begins here in window `pair`, at 0 in the next one
  const float* a = win + (long)pair * S * p.Tw + oa;
  const float* b = win + ((long)pair + 1) * S * p.Tw;
  double acc[S * S];
#pragma unroll
  for (int e = 0; e < S * S; ++e) acc[e] = 0.0;
  for (long j = j0 + threadIdx.x; j < j1; j += 256) {
    double av[S], bv[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      av[i] = (double)a[(long)i * p.Tw + j];
      bv[i] = (double)b[(long)i * p.Tw + j];
    }
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int q = 0; q < S; ++q) acc[i * S + q] += av[i] * bv[q];
  }
  const double r = ds_block_totals_d<4, S * S>(acc, S * S, sh);
  if (threadIdx.x < S * S) part[((long)pair * kLfBlocks + blk) * (S * S) + threadIdx.x] = r;
}

// cmat[pair][S][S] (and gram_out) = the block partials summed in order; then thread 0 chains the permutations.  grid (1), 256 threads
__global__ __launch_bounds__(256) void lf_perm_kernel(const double* __restrict__ part, double* __restrict__ cmat,
                                                      double* __restrict__ gram_out, int* __restrict__ perm_out, int K, int S) {
  const int SS = S * S;
  for (long e = threadIdx.x; e < (long)(K - 1) * SS; e += 256) {
    const long pair = e / SS;
    const int ij = (int)(e % SS);
    double s = 0.0;
    for (int blk = 0; blk < kLfBlocks; ++blk) s += part[(pair * kLfBlocks + blk) * SS + ij];
    cmat[e] = s;
    if (gram_out) gram_out[e] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int g[kLfMaxS];
  for (int i = 0; i < S; ++i) { g[i] = i; perm_out[i] = i; }
  for (int k = 0; k + 1 < K; ++k) {
    const int best = ds_best_perm(cmat + (long)k * SS, S);
    int gn[kLfMaxS];
    for (int i = 0; i < S; ++i) gn[i] = ds_perm_entry(S, best, g[i]);
    for (int i = 0; i < S; ++i) { g[i] = gn[i]; perm_out[(long)(k + 1) * S + i] = gn[i]; }
  }
}

// a + (b - a) r, r = (j + 0.5) / n: one float32 rounding per operation (no contraction into an fma; the division is the
// correctly rounded one), so a == b gives a
__device__ inline float lf_fade(float a, float b, long j, long n) {
#pragma clang fp contract(off)
  const float r = ((float)j + 0.5f) / (float)n;
  const float d = b - a;
  const float dr = d * r;
  return a + dr;
}

// out[i][t].  grid (ceil(T / 256), S), 256 threads
__global__ __launch_bounds__(256) void lf_blend_kernel(const float* __restrict__ win, const int* __restrict__ perm,
                                                       float* __restrict__ out, LfPlan p, int S) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.T) return;
  const int i = blockIdx.y;
  int k;
  long j, n;
  lf_locate(p, t, &k, &j, &n);
  int ra = perm[(long)k * S + i];
  ra = ra < 0 ? 0 : (ra >= S ? S - 1 : ra);
  const float a = win[((long)k * S + ra) * p.Tw + (t - lf_start(p, k))];
  float v = a;
  if (n > 0) {
    int rb = perm[((long)k + 1) * S + i];
    rb = rb < 0 ? 0 : (rb >= S ? S - 1 : rb);
    const float b = win[(((long)k + 1) * S + rb) * p.Tw + (t - lf_start(p, k + 1))];
    v = lf_fade(a, b, j, n);
  }
  out[(long)i * p.T + t] = v;
}

int64_t lf_workspace(int K, int S) {
  const int64_t pairs = K > 1 ? K - 1 : 1;
  return (pairs * (kLfBlocks + 1) * S * S * 8 + 255) / 256 * 256;
}

}  // namespace

extern "C" int32_t diffsep_longform_plan(int64_t T, int64_t Tw, int64_t Tv, int64_t* starts_out, int32_t cap) {
  LfPlan p;
  const std::string why = lf_make_plan(T, Tw, Tv, &p);
  if (!why.empty()) {
    ds_set_error("longform_plan: " + why);
    return -1;
  }
  if (starts_out) {
    if (cap < p.K) {
      ds_set_error("longform_plan: cap = " + std::to_string(cap) + " < K = " + std::to_string(p.K) + " windows");
      return -1;
    }
    for (int k = 0; k < p.K; ++k) starts_out[k] = lf_start(p, k);
  }
  return p.K;
}

extern "C" int32_t diffsep_longform_locate(int64_t T, int64_t Tw, int64_t Tv, int64_t t, int32_t* k_out, int64_t* j_out,
                                           int64_t* n_out) {
  LfPlan p;
  const std::string why = lf_make_plan(T, Tw, Tv, &p);
  DS_CHECK(why.empty(), "longform_locate: " + why);
  DS_CHECK(t >= 0 && t < T, "longform_locate: t = " + std::to_string(t) + " outside [0, T)");
  DS_CHECK(k_out && j_out && n_out, "longform_locate: null pointer");
  int k;
  long j, n;
  lf_locate(p, t, &k, &j, &n);
  *k_out = k; *j_out = j; *n_out = n;
  return 0;
}

extern "C" int64_t diffsep_longform_workspace_bytes(int32_t K, int32_t S) {
  if (K < 1 || S < 1 || S > kLfMaxS) {
    ds_set_error("longform_workspace_bytes: bad shape K=" + std::to_string(K) + " S=" + std::to_string(S) + " (K >= 1, S in 1..3)");
    return -1;
  }
  return lf_workspace(K, S);
}

extern "C" int32_t diffsep_longform_stitch(const float* win, int32_t K, int32_t S, int64_t Tw, int64_t T, int64_t Tv, float* out,
                                           int32_t* perm_out, double* gram_out, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
  LfPlan p;
  DS_CHECK(win && out && perm_out && workspace, "longform_stitch: null pointer");
  DS_CHECK(S >= 1 && S <= kLfMaxS, "longform_stitch: S = " + std::to_string(S) + " sources (1..3)");
  const std::string why = lf_make_plan(T, Tw, Tv, &p);
  DS_CHECK(why.empty(), "longform_stitch: " + why);
  DS_CHECK(K == p.K, "longform_stitch: K = " + std::to_string(K) + " windows, the plan of T = " + std::to_string(T) + ", Tw = " +
                         std::to_string(Tw) + ", Tv = " + std::to_string(Tv) + " has " + std::to_string(p.K));
  DS_CHECK(workspace_bytes >= lf_workspace(K, S), "longform_stitch: workspace too small (" + std::to_string(workspace_bytes) +
                                                      " < " + std::to_string(lf_workspace(K, S)) + " bytes)");
  DS_CHECK(((uintptr_t)workspace & 7) == 0, "longform_stitch: workspace must be 8-byte aligned");
  DS_CHECK((T + 255) / 256 < ((int64_t)1 << 31), "longform_stitch: T too long for one launch");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  double* cmat = part + (long)(K > 1 ? K - 1 : 1) * kLfBlocks * S * S;
  if (K > 1) {
    const unsigned nb = (unsigned)(K - 1) * kLfBlocks;
    if (S == 1) lf_gram_kernel<1><<<nb, 256, 0, st>>>(win, part, p);
    else if (S == 2) lf_gram_kernel<2><<<nb, 256, 0, st>>>(win, part, p);
    else lf_gram_kernel<3><<<nb, 256, 0, st>>>(win, part, p);
    DS_LAUNCH_CHECK();
  }
  lf_perm_kernel<<<1, 256, 0, st>>>(part, cmat, gram_out, perm_out, K, S);
  DS_LAUNCH_CHECK();
  lf_blend_kernel<<<dim3((unsigned)((T + 255) / 256), S), 256, 0, st>>>(win, perm_out, out, p, S);
  DS_LAUNCH_CHECK();
  return 0;
}
