// bss_eval.hip — BSS-eval SDR / SIR / SAR with a time-invariant distortion filter of L taps for every utterance of a zero-padded
// batch on the device, float64 from the fp32 samples on (mir_eval.separation.bss_eval_sources; fast_bss_eval.bss_eval_sources(ref,
// est, filter_length=L), the package the reference's evaluate.py:103-132 imports for the SI forms).
//
// Per utterance, references r_0 .. r_{S-1}, estimates e_0 .. e_{S-1}, n = lengths[b] samples.  A_i: the (n + L - 1) x L matrix
// whose column tau is r_i delayed by tau; A = [A_0 ... A_{S-1}]; P_i, P the orthogonal projections onto their column spans:
//   s_target = P_i e_j,  e_interf = P e_j - P_i e_j,  e_artif = e_j - P e_j.
// Everything follows from correlations X(x, y, l) = sum_m x[m] y[m + l], 0 <= l < L:
//   R[(i, tau), (k, tau')] = c_ik(tau - tau'),  c_ik(l) = X(r_i, r_k, l) (l >= 0) = X(r_k, r_i, -l) (l < 0);   S L x S L
//   b_j[(i, tau)] = X(r_i, e_j, tau);   E_j = X(e_j, e_j, 0)
//   q_ij = b_ij^T R_ii^-1 b_ij,   Q_j = b_j^T R^-1 b_j
//   SDR[i][j] = 10 log10(q_ij / (E_j - q_ij)),  SIR[i][j] = 10 log10(q_ij / (Q_j - q_ij)),  SAR[j] = 10 log10(Q_j / (E_j - Q_j))
// (span(A_i) is inside span(A), so |P e - P_i e|^2 = Q - q).  Rules: a denominator <= 0 is +inf; a non-positive Cholesky pivot
// makes every value of that factorisation NaN (R_ii: row i of SDR and SIR; R: every SIR and SAR); clamp_db > 0 clamps what is
// not NaN to [-clamp_db, clamp_db].
//
// Systems of an utterance: system 0 is R (order S L), systems 1 .. S-1 are the diagonal blocks R_11 .. R_{S-1,S-1} (order L);
// R_00 is the leading block of R, so chol(R_00) is the leading block of chol(R) and q_0j is the first L terms of Q_j's sum.
// A system of order N is stored column-major with N + S rows: rows N .. N + S - 1 are the right-hand sides b_j^T.  The blocked
// right-looking Cholesky treats them as more rows of the lower triangle: the panel solve that turns A[i][k] into L[i][k] turns
// b_j^T into (L^-1 b_j)^T, the forward substitution, and Q_j is the sum of its squares.
//
// Launch sequence (no host loop over utterances, no readback; the loop over panels depends on S and L alone):
//   bss_corr_kernel     per (time chunk of 2048 samples, correlation job, utterance): L lags of one pair of rows, 4 lags per
//                       thread, the chunk split among 256 / ceil(L / 4) thread groups and their sums folded first to last
//   bss_reduce_kernel   per (job, utterance): the chunks' sums first to last
//   bss_fill_kernel     per (system, utterance): the Toeplitz blocks and the right-hand sides from the correlations
//   per panel of 64 columns:
//     bss_panel_kernel  per (256 rows below the panel, system): the 64 x 64 diagonal block factored in LDS (every block of a
//                       system does it, the block is never written back: nothing reads it again), then one row per thread
//                       solved against it in registers
//     bss_update_kernel per (64 x 64 tile of the lower triangle behind the panel, system): C -= P_i P_j^T
//   bss_finish_kernel   per utterance: the quadratic forms (reduce_device.h), dB values, permutation search (perm_search.h)
// The time partition is a function of n and L alone and every sum has a fixed order, no atomics: row b equals the B = 1 call
// on that utterance bit for bit, at any padded T, in any batch, on any stream.  Samples at t >= n are never read.
#include <cmath>

#include "../../include/diffsep_hip.h"
#include "common.h"
#include "pair_metrics.h"
#include "perm_search.h"
#include "reduce_device.h"

namespace {

constexpr int kNB = 64;       // panel width of the Cholesky = tile edge of the trailing update
constexpr int kCH = 2048;     // samples per time chunk of the correlation
constexpr int kMaxL = 1024;

struct BssLayout {
  int64_t njobs, nch;         // correlation jobs per utterance, chunks of T
  int64_t sys0, sys1, mat;    // doubles of system 0, of a diagonal-block system, of all systems of an utterance
  int64_t off_part, off_corr, off_mat, off_fail, total;
};

std::string bss_shape(int B, int S, int64_t T, int L) {
  return "B=" + std::to_string(B) + " S=" + std::to_string(S) + " T=" + std::to_string(T) + " L=" + std::to_string(L);
}

// empty: fine; else what is refused
std::string bss_layout(int B, int S, int64_t T, int L, BssLayout* l) {
  if (S < 1 || S > 3) return "S outside 1..3";
  if (L < 1 || L > kMaxL) return "L outside 1.." + std::to_string(kMaxL);
  if (B < 1 || (int64_t)B * S > 65535) return "B outside 1..65535 / S";
  if (T < 1 || T >= ((int64_t)1 << 31)) return "T outside 1..2^31-1";
  l->njobs = 2 * S * S + S;
  l->nch = (T + kCH - 1) / kCH;
  const int64_t N = (int64_t)S * L;
  l->sys0 = (N + S) * N;
  l->sys1 = ((int64_t)L + S) * L;
  l->mat = l->sys0 + (S - 1) * l->sys1;
  DsCarver ws;
  l->off_part = ws.take((int64_t)B * l->njobs * l->nch * L * 8);
  l->off_corr = ws.take((int64_t)B * l->njobs * L * 8);
  l->off_mat = ws.take((int64_t)B * l->mat * 8);
  l->off_fail = ws.take((int64_t)B * S * 4);
  l->total = ws.total;
  return "";
}

// ---------------------------------------------------------------------------------------------------------------- kernels
// job < S^2: X(r_a, r_b, .), a = job / S, b = job % S;  S^2 <= job < 2 S^2: X(r_a, e_b, .);  then X(e_j, e_j, 0) (one lag)
struct BssJob { int xest, xrow, yest, yrow, nl; };
__device__ inline BssJob bss_job(int job, int S, int L) {
  const int SS = S * S;
  if (job < SS) return {0, job / S, 0, job % S, L};
  if (job < 2 * SS) return {0, (job - SS) / S, 1, (job - SS) % S, L};
  return {1, job - 2 * SS, 1, job - 2 * SS, 1};
}

struct BssSys { double* M; int N, ld; };  // column-major, ld = N + S rows
__device__ inline BssSys bss_sys(double* mats, const BssLayout& l, int b, int s, int S, int L) {
  double* base = mats + (long)b * l.mat;
  if (s == 0) return {base, S * L, S * L + S};
  return {base + l.sys0 + (long)(s - 1) * l.sys1, L, L + S};
}

// part[b][job][chunk][l] = sum over the chunk's m of x[m] y[m + l].  grid (chunks of T, jobs, B), 256 threads
__global__ __launch_bounds__(256) void bss_corr_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                       const int* __restrict__ lengths, double* __restrict__ part, int S,
                                                       long T, int L, BssLayout lay) {
  __shared__ __attribute__((aligned(16))) float xs[kCH];
  __shared__ __attribute__((aligned(16))) float ys[kCH + kMaxL + 16];
  __shared__ double gs[256 * 4];
  const int ch = blockIdx.x, job = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  const int n = ds_pair_len(lengths, b, T);
  const long c0 = (long)ch * kCH;
  if (c0 >= n) return;  // (the whole block)
  const BssJob j = bss_job(job, S, L);
  const float* x = (j.xest ? est : ref) + ((long)b * S + j.xrow) * T;
  const float* y = (j.yest ? est : ref) + ((long)b * S + j.yrow) * T;
  const int nlq = (j.nl + 3) >> 2;  // quads of lags, <= 256
  const int ngr = 256 / nlq;        // thread groups, each with a share of the chunk
  const int ylen = kCH + 4 * nlq + 8;
  for (int i = t; i < kCH; i += 256) xs[i] = c0 + i < n ? x[c0 + i] : 0.0f;
  for (int i = t; i < ylen; i += 256) ys[i] = c0 + i < n ? y[c0 + i] : 0.0f;
  __syncthreads();
  const int g = t / nlq, lq = t - g * nlq;
  const int sub = (((kCH + ngr - 1) / ngr) + 3) & ~3;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (g < ngr) {
    const int m0 = g * sub, m1 = min(kCH, m0 + sub);
    const float4* x4 = reinterpret_cast<const float4*>(xs);
    const float4* y4 = reinterpret_cast<const float4*>(ys) + lq;
    if (m0 < m1) {
      float4 v = y4[m0 >> 2];
      double w0 = (double)v.x, w1 = (double)v.y, w2 = (double)v.z, w3 = (double)v.w;
      for (int m = m0; m < m1; m += 4) {
        const float4 xv = x4[m >> 2];
        v = y4[(m >> 2) + 1];
        const double x0 = (double)xv.x, x1 = (double)xv.y, x2 = (double)xv.z, x3 = (double)xv.w;
        const double w4 = (double)v.x, w5 = (double)v.y, w6 = (double)v.z, w7 = (double)v.w;
        a0 = fma(x0, w0, a0); a1 = fma(x0, w1, a1); a2 = fma(x0, w2, a2); a3 = fma(x0, w3, a3);
        a0 = fma(x1, w1, a0); a1 = fma(x1, w2, a1); a2 = fma(x1, w3, a2); a3 = fma(x1, w4, a3);
        a0 = fma(x2, w2, a0); a1 = fma(x2, w3, a1); a2 = fma(x2, w4, a2); a3 = fma(x2, w5, a3);
        a0 = fma(x3, w3, a0); a1 = fma(x3, w4, a1); a2 = fma(x3, w5, a2); a3 = fma(x3, w6, a3);
        w0 = w4; w1 = w5; w2 = w6; w3 = w7;
      }
    }
  }
  gs[t * 4] = a0; gs[t * 4 + 1] = a1; gs[t * 4 + 2] = a2; gs[t * 4 + 3] = a3;  // t = g nlq + lq
  __syncthreads();
  double* o = part + (((long)b * lay.njobs + job) * lay.nch + ch) * L;
  for (int l = t; l < j.nl; l += 256) {
    double s = gs[l];  // group 0: (0 nlq + l / 4) 4 + l % 4
    for (int q = 1; q < ngr; ++q) s += gs[q * nlq * 4 + l];
    o[l] = s;
  }
}

// corr[b][job][l] = the chunks' sums, first to last.  grid (jobs, B), 256 threads
__global__ __launch_bounds__(256) void bss_reduce_kernel(const double* __restrict__ part, const int* __restrict__ lengths,
                                                         double* __restrict__ corr, int S, long T, int L, BssLayout lay) {
  const int job = blockIdx.x, b = blockIdx.y;
  const int n = ds_pair_len(lengths, b, T);
  const int nch = (n + kCH - 1) / kCH, nl = bss_job(job, S, L).nl;
  const double* p = part + ((long)b * lay.njobs + job) * lay.nch * L;
  for (int l = threadIdx.x; l < nl; l += 256) {
    double s = 0.0;
    for (int c = 0; c < nch; ++c) s = c == 0 ? p[l] : s + p[(long)c * L + l];
    corr[((long)b * lay.njobs + job) * L + l] = s;
  }
}

// the systems of an utterance from its correlations; fail[b][s] = N (no failed pivot).  grid (blocks, S, B), 256 threads
__global__ __launch_bounds__(256) void bss_fill_kernel(const double* __restrict__ corr, double* __restrict__ mats,
                                                       int* __restrict__ fail, int S, int L, BssLayout lay) {
  const int s = blockIdx.y, b = blockIdx.z;
  const BssSys m = bss_sys(mats, lay, b, s, S, L);
  const double* G = corr + (long)b * lay.njobs * L;  // [job][L]
  if (blockIdx.x == 0 && threadIdx.x == 0) fail[b * S + s] = m.N;
  const long total = (long)m.ld * m.N;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int c = (int)(e / m.ld), r = (int)(e - (long)c * m.ld);
    const int ci = s == 0 ? c / L : s, ct = s == 0 ? c - (c / L) * L : c;
    double v;
    if (r < m.N) {
      const int ri = s == 0 ? r / L : s, rt = s == 0 ? r - (r / L) * L : r;
      const int lag = rt - ct;
      v = lag >= 0 ? G[(long)(ri * S + ci) * L + lag] : G[(long)(ci * S + ri) * L - lag];
    } else {
      v = G[(long)(S * S + ci * S + (r - m.N)) * L + ct];
    }
    m.M[e] = v;
  }
}

// Panel k0 .. k0 + nb - 1 of every system that has it: rows below the diagonal block become L[i][k] (right-hand sides: their
// forward substitution).  fail[b][s]: the first non-positive pivot (it is replaced by 1 so that the arithmetic goes on; what
// depends on it is NaN in the end).  grid (256-row groups of system 0, B * S), 256 threads
__global__ __launch_bounds__(256) void bss_panel_kernel(double* __restrict__ mats, int* __restrict__ fail, int S, int L, int k0,
                                                        BssLayout lay) {
  __shared__ double Lk[kNB][kNB + 1];  // [row][column] of the diagonal block, lower triangle
  __shared__ double diag[kNB];
  const int b = blockIdx.y / S, s = blockIdx.y - b * S, t = threadIdx.x;
  const BssSys m = bss_sys(mats, lay, b, s, S, L);
  if (k0 >= m.N) return;
  const int nb = min(kNB, m.N - k0);
  const int row0 = k0 + nb + blockIdx.x * 256;
  if (row0 >= m.ld) return;
  for (int e = t; e < kNB * kNB; e += 256) {
    const int c = e >> 6, r = e & 63;
    double v = r == c ? 1.0 : 0.0;  // beyond nb: the identity
    if (r < nb && c <= r) v = m.M[(long)(k0 + c) * m.ld + k0 + r];
    Lk[r][c] = v;
  }
  if (t < kNB) diag[t] = 1.0;
  int failc = -1;
  const int ur = t & 63, uq = t >> 6;
  for (int c = 0; c < nb; ++c) {
    __syncthreads();
    double d = Lk[c][c];
    if (!(d > 0.0)) {
      if (failc < 0) failc = c;
      d = 1.0;
    }
    const double sq = sqrt(d);
    if (t == 0) diag[c] = sq;
    if (t > c && t < nb) Lk[t][c] /= sq;
    __syncthreads();
    if (ur > c && ur < nb) {
      const double lr = Lk[ur][c];
      for (int q = c + 1 + uq; q <= ur; q += 4) Lk[ur][q] = fma(-lr, Lk[q][c], Lk[ur][q]);
    }
  }
  __syncthreads();
  if (blockIdx.x == 0 && t == 0 && failc >= 0 && fail[b * S + s] == m.N) fail[b * S + s] = k0 + failc;
  const int r = row0 + t;
  if (r >= m.ld) return;
  double* p = m.M + (long)k0 * m.ld + r;
  // x L_kk^T = a for this row, 16 columns in registers at a time: first the columns already solved (read back: this thread
  // wrote them), then the 16 x 16 triangle.  Beyond nb the block is the identity and nothing is stored.
  for (int cb = 0; cb < nb; cb += 16) {
    double x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = cb + i < nb ? p[(long)(cb + i) * m.ld] : 0.0;
    for (int q = 0; q < cb; ++q) {
      const double xq = p[(long)q * m.ld];
#pragma unroll
      for (int i = 0; i < 16; ++i) x[i] = fma(-xq, Lk[cb + i][q], x[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      double acc = x[i];
#pragma unroll
      for (int k = 0; k < i; ++k) acc = fma(-x[k], Lk[cb + i][cb + k], acc);
      x[i] = acc / diag[cb + i];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (cb + i < nb) p[(long)(cb + i) * m.ld] = x[i];
  }
}

// C[r][c] -= sum_p P[r][p] P[c][p] over the 64 columns of panel k0, for the tiles (it >= jt) of the lower triangle behind it,
// right-hand-side rows included.  grid (tiles of system 0, B * S), 256 threads, 4 x 4 results each
__global__ __launch_bounds__(256) void bss_update_kernel(double* __restrict__ mats, int S, int L, int k0, BssLayout lay) {
  __shared__ __attribute__((aligned(16))) double Pi[kNB][kNB];  // [p][row of the tile]
  __shared__ __attribute__((aligned(16))) double Pj[kNB][kNB];  // [p][column of the tile]
  const int b = blockIdx.y / S, s = blockIdx.y - b * S, t = threadIdx.x;
  const BssSys m = bss_sys(mats, lay, b, s, S, L);
  const int r0 = k0 + kNB;
  if (r0 >= m.N) return;
  const int mt = (m.ld - r0 + kNB - 1) / kNB, nt = (m.N - r0 + kNB - 1) / kNB;
  int idx = blockIdx.x, jt = 0;
  while (jt < nt && idx >= mt - jt) { idx -= mt - jt; ++jt; }
  if (jt >= nt) return;
  const int rbase = r0 + (jt + idx) * kNB, cbase = r0 + jt * kNB;
  const double* P = m.M + (long)k0 * m.ld;
  for (int e = t; e < kNB * kNB; e += 256) {
    const int p = e >> 6, i = e & 63;
    Pi[p][i] = rbase + i < m.ld ? P[(long)p * m.ld + rbase + i] : 0.0;
    Pj[p][i] = cbase + i < m.N ? P[(long)p * m.ld + cbase + i] : 0.0;
  }
  __syncthreads();
  const int tx = (t & 15) * 4, ty = (t >> 4) * 4;
  double acc[4][4] = {};
  for (int p = 0; p < kNB; ++p) {
    double ra[4], cb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { ra[i] = Pi[p][tx + i]; cb[i] = Pj[p][ty + i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[i][k] = fma(ra[i], cb[k], acc[i][k]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = cbase + ty + k;
    if (c >= m.N) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = rbase + tx + i;
      if (r < m.ld) m.M[(long)c * m.ld + r] -= acc[i][k];
    }
  }
}

// sum of the squares of row `row` of a system over its first cnt columns, to every thread
__device__ inline double bss_sumsq(const BssSys& m, int row, int cnt, double* sh4) {
  double part = 0.0;
  for (int c = threadIdx.x; c < cnt; c += 256) {
    const double v = m.M[(long)c * m.ld + row];
    part = fma(v, v, part);
  }
  return ds_block_sum_d<4>(part, sh4);
}

__device__ inline double bss_db(double num, double den, double clamp) {
  double v = den <= 0.0 ? __longlong_as_double(0x7ff0000000000000LL) : 10.0 * log10(num / den);
  if (clamp > 0.0 && v == v) v = fmin(fmax(v, -clamp), clamp);
  return v;
}

// grid (B), 256 threads
__global__ __launch_bounds__(256) void bss_finish_kernel(double* __restrict__ mats, const double* __restrict__ corr,
                                                         const int* __restrict__ fail, const int* __restrict__ perm,
                                                         double* __restrict__ out, double* __restrict__ pair_out,
                                                         int* __restrict__ perm_out, int S, int L, double clamp, BssLayout lay) {
  __shared__ double sh4[4];
  const int b = blockIdx.x, N = S * L;
  const BssSys m0 = bss_sys(mats, lay, b, 0, S, L);
  double Q[3], q[3][3];
  for (int j = 0; j < S; ++j) {
    Q[j] = bss_sumsq(m0, N + j, N, sh4);
    q[0][j] = bss_sumsq(m0, N + j, L, sh4);  // S = 1: the same sum as Q
    for (int i = 1; i < S; ++i) q[i][j] = bss_sumsq(bss_sys(mats, lay, b, i, S, L), L + j, L, sh4);
  }
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL), ninf = __longlong_as_double(0xfff0000000000000LL);
  const int f0 = fail[b * S];
  const bool bad_all = f0 < N;
  double sdr[9], sir[9], sar[3], cost[9];
  for (int j = 0; j < S; ++j) {
    const double E = corr[((long)b * lay.njobs + 2 * S * S + j) * L];
    sar[j] = bad_all ? nan : bss_db(Q[j], E - Q[j], clamp);
    for (int i = 0; i < S; ++i) {
      const bool bad = i == 0 ? f0 < L : fail[b * S + i] < L;
      sdr[i * S + j] = bad ? nan : bss_db(q[i][j], E - q[i][j], clamp);
      sir[i * S + j] = bad || bad_all ? nan : bss_db(q[i][j], Q[j] - q[i][j], clamp);
      cost[i * S + j] = sdr[i * S + j] == sdr[i * S + j] ? sdr[i * S + j] : ninf;  // NaN counts as -inf
    }
  }
  const int best = perm ? 0 : ds_best_perm(cost, S);
  for (int i = 0; i < S; ++i) {
    int pj;
    if (perm) {
      pj = perm[b * S + i];
      pj = pj < 0 ? 0 : (pj >= S ? S - 1 : pj);
    } else {
      pj = ds_perm_entry(S, best, i);
    }
    out[((long)b * 3 + 0) * S + i] = sdr[i * S + pj];
    out[((long)b * 3 + 1) * S + i] = sir[i * S + pj];
    out[((long)b * 3 + 2) * S + i] = sar[pj];
    if (perm_out) perm_out[b * S + i] = pj;
  }
  if (pair_out)
    for (int e = 0; e < S * S; ++e) {
      pair_out[((long)b * 2 + 0) * S * S + e] = sdr[e];
      pair_out[((long)b * 2 + 1) * S * S + e] = sir[e];
    }
}

}  // namespace

extern "C" int64_t diffsep_bss_eval_workspace_bytes(int32_t B, int32_t S, int64_t T, int32_t L) {
  BssLayout l;
  const std::string why = bss_layout(B, S, T, L, &l);
  if (!why.empty()) {
    ds_set_error("bss_eval_workspace_bytes: " + why + " (" + bss_shape(B, S, T, L) + ")");
    return -1;
  }
  return l.total;
}

extern "C" int32_t diffsep_bss_eval(const float* ref, const float* est, double* out, double* pair_out, int32_t* perm_out,
                                    int32_t B, int32_t S, int64_t T, const int32_t* lengths, const int32_t* perm, int32_t L,
                                    double clamp_db, void* workspace, int64_t workspace_bytes, void* stream) {
  BssLayout l;
  const std::string why = bss_layout(B, S, T, L, &l);
  DS_CHECK(why.empty(), "bss_eval: " + why + " (" + bss_shape(B, S, T, L) + ")");
  DS_CHECK(ref, "bss_eval: ref is null");
  DS_CHECK(est, "bss_eval: est is null");
  DS_CHECK(out, "bss_eval: out is null");
  DS_CHECK(workspace, "bss_eval: workspace is null");
  DS_CHECK(clamp_db >= 0.0, "bss_eval: clamp_db must be >= 0 (0: no clamp)");
  DS_CHECK(workspace_bytes >= l.total, "bss_eval: workspace_bytes " + std::to_string(workspace_bytes) + " < " +
                                           std::to_string(l.total) + " (" + bss_shape(B, S, T, L) + ")");
  DS_CHECK(((uintptr_t)workspace & 7) == 0, "bss_eval: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* part = (double*)(ws + l.off_part);
  double* corr = (double*)(ws + l.off_corr);
  double* mats = (double*)(ws + l.off_mat);
  int* fail = (int*)(ws + l.off_fail);
  const int N = S * L, ld = N + S;
  bss_corr_kernel<<<dim3((unsigned)l.nch, (unsigned)l.njobs, B), 256, 0, st>>>(ref, est, lengths, part, S, T, L, l);
  DS_LAUNCH_CHECK();
  bss_reduce_kernel<<<dim3((unsigned)l.njobs, B), 256, 0, st>>>(part, lengths, corr, S, T, L, l);
  DS_LAUNCH_CHECK();
  const unsigned fill_blocks = (unsigned)std::min<int64_t>(256, (l.sys0 + 255) / 256);
  bss_fill_kernel<<<dim3(fill_blocks, S, B), 256, 0, st>>>(corr, mats, fail, S, L, l);
  DS_LAUNCH_CHECK();
  for (int k0 = 0; k0 < N; k0 += kNB) {
    const int nb = std::min(kNB, N - k0);
    bss_panel_kernel<<<dim3((ld - k0 - nb + 255) / 256, B * S), 256, 0, st>>>(mats, fail, S, L, k0, l);
    DS_LAUNCH_CHECK();
    const int r0 = k0 + kNB;
    if (r0 < N) {
      const int mt = (ld - r0 + kNB - 1) / kNB, nt = (N - r0 + kNB - 1) / kNB;
      bss_update_kernel<<<dim3(nt * mt - nt * (nt - 1) / 2, B * S), 256, 0, st>>>(mats, S, L, k0, l);
      DS_LAUNCH_CHECK();
    }
  }
  bss_finish_kernel<<<B, 256, 0, st>>>(mats, corr, fail, perm, out, pair_out, perm_out, S, L, clamp_db, l);
  DS_LAUNCH_CHECK();
  return 0;
}
