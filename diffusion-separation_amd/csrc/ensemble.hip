// ensemble.hip — K posterior draws of every utterance of a zero-padded batch, aligned to one source order and reduced on the
// device: mean, spread, distance of every draw to the mean, and the medoid draw (diffsep_ensemble; the reference has no
// counterpart: it returns one draw per call).
//
// draws [B][K][S][T], anchor [B][S][T] or draw 0 of each utterance, n = lens[b] (<= T).  Every launch is asynchronous, nothing
// is read back, there are no floating-point atomics.  An utterance's time axis is cut into kEnsParts contiguous shares of
// ens_share(n) samples — a function of n alone, a multiple of 4 — one block per share, and a thread of a block takes the groups
// of 4 consecutive samples g, g + 256, ... of its share, the samples of a group in order.  So what is computed for utterance b
// depends on n and on its own samples only: not on B, b, the padded width T or the stream.  A group that lies inside n on a
// 16-byte aligned row is fetched (stored) with one 16-byte access, any other group sample by sample with t < n checked; both
// paths hand the same four values to the same arithmetic (ens_load4 / ens_store4), so they give the same bits.
//   ens_gram_kernel   block (share, k, b): partial sums of C[k][i][j] = sum_t (double)a[i][t] (double)d[k][j][t] (products of
//                     two floats are exact in float64), block totals in the fixed order of reduce_device.h
//   ens_perm_kernel   block b: C = the kEnsParts partials of every entry folded in share order; r_k by the rule of
//                     perm_search.h (with the anchor defaulted to draw 0, r_0 = identity without a search); gram_out, perm_out
//   ens_reduce_kernel block (share, i, b): per sample m = (((v_0 + v_1) + ...) + v_{K-1}) / K with v_k = d[k][r_k[i]], then k
//                     ascending q = (v_k - m)^2 (each operation rounded on its own: no contraction) into the spread's sum and
//                     into the block's partial of dist[k]; mean_out, std_out, zeros from n to T; draws 8 at a time, so the
//                     partial sums live in registers whatever K is
//   ens_final_kernel  block b: dist[k] = the partials folded source-major, share-minor; medoid = first minimum
//   ens_pick_kernel   block (share, i, b): pick_out = v_medoid, zeros from n to T (only when pick_out is asked for)
#include <string>

#include "../../include/diffsep_hip.h"
#include "common.h"
#include "perm_search.h"    // the permutation rule (lexicographic candidates, strict >), shared with longform.hip
#include "reduce_device.h"  // the fixed-order fp64 block totals

namespace {

constexpr int kEnsParts = 32;  // shares (= blocks, = partial sums) per utterance and draw: B = 16, K = 4 is 2048 blocks of the Gram pass
constexpr int kEnsMaxS = 3;
constexpr int kEnsMaxK = 32;
constexpr int kEnsKG = 8;      // draws whose distance partials a thread of the reduce pass holds at a time

__host__ __device__ inline long ens_share(long n) { return ((n + kEnsParts - 1) / kEnsParts + 3) / 4 * 4; }

__device__ inline int ens_len(const int* lens, int b, long T) {
  if (!lens) return (int)T;
  const int n = lens[b];
  return n < 0 ? 0 : (n > T ? (int)T : n);
}

// the four samples t .. t + 3 of a row (those at or beyond n are not read and come back as 0)
__device__ inline void ens_load4(const float* __restrict__ row, long t, long n, bool vec, float* v) {
  if (vec && t + 4 <= n) {
    const float4 q = *reinterpret_cast<const float4*>(row + t);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = t + e < n ? row[t + e] : 0.0f;
  }
}
__device__ inline void ens_store4(float* __restrict__ row, long t, long n, bool vec, const float* v) {
  if (vec && t + 4 <= n) {
    *reinterpret_cast<float4*>(row + t) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (t + e < n) row[t + e] = v[e];
  }
}
// row[n .. T) = +0.0, the kEnsParts blocks of the row each a contiguous piece
__device__ inline void ens_zero_tail(float* __restrict__ row, long n, long T, int part) {
  const long piece = (T - n + kEnsParts - 1) / kEnsParts;
  const long t0 = n + (long)part * piece, t1 = t0 + piece < T ? t0 + piece : T;
  for (long t = t0 + threadIdx.x; t < t1; t += 256) row[t] = 0.0f;
}
__device__ inline int ens_clamp(int r, int S) { return r < 0 ? 0 : (r >= S ? S - 1 : r); }

// part[b][k][share][S][S].  grid (kEnsParts, K, B), 256 threads
template <int S>
__global__ __launch_bounds__(256) void ens_gram_kernel(const float* __restrict__ draws, const float* __restrict__ anchor,
                                                       const int* __restrict__ lens, double* __restrict__ part, int K, long T,
                                                       int vec) {
  __shared__ double sh[S * S][4];
  const int p = blockIdx.x, k = blockIdx.y, b = blockIdx.z;
  const long n = ens_len(lens, b, T);
  const long share = ens_share(n);
  const long t0 = (long)p * share, t1 = t0 + share < n ? t0 + share : n;
  const float* a = anchor ? anchor + (long)b * S * T : draws + (long)b * K * S * T;
  const float* d = draws + ((long)b * K + k) * S * T;
  double acc[S * S];
#pragma unroll
  for (int e = 0; e < S * S; ++e) acc[e] = 0.0;
  for (long t = t0 + 4 * (long)threadIdx.x; t < t1; t += 4 * 256) {
    float av[S][4], dv[S][4];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      ens_load4(a + (long)i * T, t, n, vec != 0, av[i]);
      ens_load4(d + (long)i * T, t, n, vec != 0, dv[i]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < S; ++i)
#pragma unroll
        for (int j = 0; j < S; ++j) acc[i * S + j] += (double)av[i][e] * (double)dv[j][e];
  }
  const double r = ds_block_totals_d<4, S * S>(acc, S * S, sh);
  if (threadIdx.x < S * S) part[(((long)b * K + k) * kEnsParts + p) * (S * S) + threadIdx.x] = r;
}

// grid (B), 256 threads
__global__ __launch_bounds__(256) void ens_perm_kernel(const double* __restrict__ part, double* __restrict__ gram_out,
                                                       int* __restrict__ perm_out, int K, int S, int self_anchor) {
  __shared__ double cm[kEnsMaxK * kEnsMaxS * kEnsMaxS];
  const int b = blockIdx.x, SS = S * S;
  for (int e = threadIdx.x; e < K * SS; e += 256) {
    const double* q = part + ((long)b * K + e / SS) * kEnsParts * SS + e % SS;
    double s = q[0];
    for (int p = 1; p < kEnsParts; ++p) s += q[(long)p * SS];
    cm[e] = s;
    if (gram_out) gram_out[(long)b * K * SS + e] = s;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= K) return;
  const int best = (self_anchor && k == 0) ? 0 : ds_best_perm(cm + k * SS, S);
  for (int i = 0; i < S; ++i) perm_out[((long)b * K + k) * S + i] = ds_perm_entry(S, best, i);
}

// the arithmetic of one sample, every operation rounded on its own
__device__ inline double ens_sqdev(float v, double m) {
#pragma clang fp contract(off)
  const double d = (double)v - m;
  return d * d;
}

// dpart[b][k][i][share].  grid (kEnsParts, S, B), 256 threads
__global__ __launch_bounds__(256) void ens_reduce_kernel(const float* __restrict__ draws, const int* __restrict__ lens,
                                                         const int* __restrict__ perm, float* __restrict__ mean_out,
                                                         float* __restrict__ std_out, double* __restrict__ dpart, int K, int S,
                                                         long T, int vec) {
  __shared__ double sh[kEnsKG][4];
  __shared__ int rows[kEnsMaxK];
  const int p = blockIdx.x, i = blockIdx.y, b = blockIdx.z;
  const long n = ens_len(lens, b, T);
  const long share = ens_share(n);
  const long t0 = (long)p * share, t1 = t0 + share < n ? t0 + share : n;
  if (threadIdx.x < K) rows[threadIdx.x] = ens_clamp(perm[((long)b * K + threadIdx.x) * S + i], S);
  __syncthreads();
  const float* d = draws + (long)b * K * S * T;
  float* mo = mean_out + ((long)b * S + i) * T;
  float* so = std_out ? std_out + ((long)b * S + i) * T : nullptr;
  const double dK = (double)K;
  for (int k0 = 0; k0 < K; k0 += kEnsKG) {
    double dq[kEnsKG];
#pragma unroll
    for (int q = 0; q < kEnsKG; ++q) dq[q] = 0.0;
    for (long t = t0 + 4 * (long)threadIdx.x; t < t1; t += 4 * 256) {
      float v[4];
      double m[4];
      ens_load4(d + (long)rows[0] * T, t, n, vec != 0, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = (double)v[e];
      for (int k = 1; k < K; ++k) {
        ens_load4(d + ((long)k * S + rows[k]) * T, t, n, vec != 0, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] += (double)v[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] /= dK;
#pragma unroll
      for (int q = 0; q < kEnsKG; ++q) {
        if (k0 + q < K) {
          ens_load4(d + ((long)(k0 + q) * S + rows[k0 + q]) * T, t, n, vec != 0, v);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (t + e < n) dq[q] += ens_sqdev(v[e], m[e]);
        }
      }
      if (k0 == 0) {  // the first round also writes the outputs of its samples
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (float)m[e];
        ens_store4(mo, t, n, vec != 0, o);
        if (so) {
          double ss[4] = {0.0, 0.0, 0.0, 0.0};
          for (int k = 0; k < K; ++k) {
            ens_load4(d + ((long)k * S + rows[k]) * T, t, n, vec != 0, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) ss[e] += ens_sqdev(v[e], m[e]);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (float)sqrt(ss[e] / dK);
          ens_store4(so, t, n, vec != 0, o);
        }
      }
    }
    const int nq = K - k0 < kEnsKG ? K - k0 : kEnsKG;
    const double r = ds_block_totals_d<4, kEnsKG>(dq, nq, sh);
    if ((int)threadIdx.x < nq) dpart[(((long)b * K + k0 + threadIdx.x) * S + i) * kEnsParts + p] = r;
  }
  ens_zero_tail(mo, n, T, p);
  if (so) ens_zero_tail(so, n, T, p);
}

// grid (B), 64 threads
__global__ __launch_bounds__(64) void ens_final_kernel(const double* __restrict__ dpart, double* __restrict__ dist_out,
                                                       int* __restrict__ medoid_out, int K, int S) {
  __shared__ double dist[kEnsMaxK];
  const int b = blockIdx.x, k = threadIdx.x;
  if (k < K) {
    const double* q = dpart + ((long)b * K + k) * S * kEnsParts;
    double s = q[0];
    for (int e = 1; e < S * kEnsParts; ++e) s += q[e];
    dist[k] = s;
    dist_out[(long)b * K + k] = s;
  }
  __syncthreads();
  if (k != 0) return;
  int best = 0;
  for (int q = 1; q < K; ++q)
    if (dist[q] < dist[best]) best = q;
  medoid_out[b] = best;
}

// grid (kEnsParts, S, B), 256 threads
__global__ __launch_bounds__(256) void ens_pick_kernel(const float* __restrict__ draws, const int* __restrict__ lens,
                                                       const int* __restrict__ perm, const int* __restrict__ medoid,
                                                       float* __restrict__ pick_out, int K, int S, long T, int vec) {
  const int p = blockIdx.x, i = blockIdx.y, b = blockIdx.z;
  const long n = ens_len(lens, b, T);
  const long share = ens_share(n);
  const long t0 = (long)p * share, t1 = t0 + share < n ? t0 + share : n;
  int k = medoid[b];
  k = k < 0 ? 0 : (k >= K ? K - 1 : k);
  const float* row = draws + (((long)b * K + k) * S + ens_clamp(perm[((long)b * K + k) * S + i], S)) * T;
  float* po = pick_out + ((long)b * S + i) * T;
  for (long t = t0 + 4 * (long)threadIdx.x; t < t1; t += 4 * 256) {
    float v[4];
    ens_load4(row, t, n, vec != 0, v);
    ens_store4(po, t, n, vec != 0, v);
  }
  ens_zero_tail(po, n, T, p);
}

// doubles: part [B][K][kEnsParts][S][S], then dpart [B][K][S][kEnsParts]
int64_t ens_workspace(int B, int K, int S) {
  return ((int64_t)B * K * kEnsParts * (S * S + S) * 8 + 255) / 256 * 256;
}

std::string ens_bad_shape(int64_t B, int64_t K, int64_t S) {
  if (K < 1 || K > kEnsMaxK) return "K = " + std::to_string(K) + " draws (1..32)";
  if (S < 1 || S > kEnsMaxS) return "S = " + std::to_string(S) + " sources (1..3)";
  if (B < 1 || B > 65535) return "B = " + std::to_string(B) + " utterances (1..65535)";
  return "";
}

}  // namespace

extern "C" int64_t diffsep_ensemble_workspace_bytes(int32_t B, int32_t K, int32_t S) {
  const std::string why = ens_bad_shape(B, K, S);
  if (!why.empty()) {
    ds_set_error("ensemble_workspace_bytes: " + why);
    return -1;
  }
  return ens_workspace(B, K, S);
}

extern "C" int32_t diffsep_ensemble(const float* draws, const float* anchor, const int32_t* lengths, int32_t B, int32_t K,
                                    int32_t S, int64_t T, float* mean_out, float* std_out, float* pick_out, int32_t* perm_out,
                                    double* dist_out, int32_t* medoid_out, double* gram_out, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  const std::string why = ens_bad_shape(B, K, S);
  DS_CHECK(why.empty(), "ensemble: " + why);
  DS_CHECK(T >= 1 && T < ((int64_t)1 << 31), "ensemble: T = " + std::to_string(T) + " samples (1 .. 2^31 - 1)");
  DS_CHECK(draws, "ensemble: draws is null");
  DS_CHECK(mean_out, "ensemble: mean_out is null");
  DS_CHECK(perm_out, "ensemble: perm_out is null");
  DS_CHECK(dist_out, "ensemble: dist_out is null");
  DS_CHECK(medoid_out, "ensemble: medoid_out is null");
  DS_CHECK(workspace, "ensemble: workspace is null");
  DS_CHECK(workspace_bytes >= ens_workspace(B, K, S), "ensemble: workspace too small (workspace_bytes = " +
                                                          std::to_string(workspace_bytes) + " < " +
                                                          std::to_string(ens_workspace(B, K, S)) + ")");
  DS_CHECK(((uintptr_t)workspace & 7) == 0, "ensemble: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  // 16-byte accesses where every row starts on a 16-byte boundary: all bases aligned and T a multiple of 4
  const uintptr_t bases = (uintptr_t)draws | (uintptr_t)anchor | (uintptr_t)mean_out | (uintptr_t)std_out | (uintptr_t)pick_out;
  const int vec = (bases & 15) == 0 && T % 4 == 0;
  double* part = (double*)workspace;
  double* dpart = part + (long)B * K * kEnsParts * S * S;
  const dim3 gk(kEnsParts, K, B), gs(kEnsParts, S, B);
  if (S == 1) ens_gram_kernel<1><<<gk, 256, 0, st>>>(draws, anchor, lengths, part, K, T, vec);
  else if (S == 2) ens_gram_kernel<2><<<gk, 256, 0, st>>>(draws, anchor, lengths, part, K, T, vec);
  else ens_gram_kernel<3><<<gk, 256, 0, st>>>(draws, anchor, lengths, part, K, T, vec);
  DS_LAUNCH_CHECK();
  ens_perm_kernel<<<B, 256, 0, st>>>(part, gram_out, perm_out, K, S, anchor ? 0 : 1);
  DS_LAUNCH_CHECK();
  ens_reduce_kernel<<<gs, 256, 0, st>>>(draws, lengths, perm_out, mean_out, std_out, dpart, K, S, T, vec);
  DS_LAUNCH_CHECK();
  ens_final_kernel<<<B, 64, 0, st>>>(dpart, dist_out, medoid_out, K, S);
  DS_LAUNCH_CHECK();
  if (pick_out) {
    ens_pick_kernel<<<gs, 256, 0, st>>>(draws, lengths, perm_out, medoid_out, pick_out, K, S, T, vec);
    DS_LAUNCH_CHECK();
  }
  return 0;
}
