// composite.hip — the signal measures behind the Hu & Loizou composite scores CSIG / CBAK / COVL of a zero-padded batch on the
// device: log-likelihood ratio (LLR), weighted spectral slope (WSS) and segmental SNR, float64 from the fp32 samples on.
//
// What the reference computes per file in evaluate_covl.py (eval_composite :18-54; lpcoeff :62-95 and llr :358-408; SSNR
// :106-152; wss :155-355), exactly as diffsep_amd/metrics.py (composite) restates it:
//   frames of win = round(30 fs / 1000) samples every skip = win / 4, n = max(0, (len - win) div skip) of them, under the
//   window 0.5 (1 - cos(2 pi j / (win + 1))), j = 1 .. win; fs = 16000: win 480, 1024-point spectrum, LPC order 16; fs = 8000:
//   240, 512, 10.  The reference's float32 casts of the autocorrelation, the LPC vector and the quadratic forms, and its float32
//   mean removal / rescaling in SSNR, are not reproduced: everything here is float64.
//
// One pair = (utterance b, reference row i, estimate row perm[b][i]).  Launch sequence (no host loop over utterances, no
// readback):
//   comp_stats_kernel   per pair and signal: mean over the len samples, then max |x - mean| (SSNR's preprocessing)
//   comp_frame_kernel   per frame of a pair: both windowed frames to LDS; segmental SNR of the mean-free, rescaled frames;
//                       autocorrelation lags 0 .. P of both, Levinson-Durbin, the two quadratic forms -> LLR; a direct
//                       float64 DFT of the bins the critical-band filters reach (twiddles from the host-built table, one
//                       spectrum per signal: an all-zero frame gives exactly zero bins), 25 band energies in dB, slopes,
//                       nearest-peak search, Klatt weights -> WSS
//   comp_final_kernel   per pair: rank of every frame's LLR and WSS (ties by frame index) -> sorted lists, the sequential
//                       ascending sum of the m = rint(0.95 n) smallest, the sequential sum of the segmental SNRs
// Every reduction has a fixed order that depends on the pair's own length only (reduce_device.h; no atomics): row (b, i) of a
// batch equals the B = 1 call bit for bit, on any stream.  Pair addressing, workspace carving, the table cache and the boundary
// checks are those of every measure on pairs: pair_metrics.h.
#include <cmath>

#include "../../include/diffsep_hip.h"
#include "common.h"
#include "pair_metrics.h"
#include "reduce_device.h"

namespace {

constexpr int kCrit = 25, kMaxWin = 480, kMaxFft = 1024, kMaxP = 16;
constexpr long kMaxFrames = 65536;  // frames per row the quadratic ranking of comp_final_kernel is offered
constexpr double kKmax = 20.0, kKlocmax = 1.0;

// critical-band filters (evaluate_covl.py:175-228): centre frequency and bandwidth in Hz
const double kCent[kCrit] = {50.0,    120.0,   190.0,   260.0,   330.0,   400.0,   470.0,   540.0,   617.372,
                             703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54, 1610.70, 1794.16,
                             1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
const double kBand[kCrit] = {70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    77.3724, 86.0056,
                             95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457, 199.776,
                             217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136};

struct CompRate { int fs, win, skip, nfft, P; };

bool comp_rate(int fs, CompRate* r) {
  if (fs == 16000) { *r = {16000, 480, 120, 1024, 16}; return true; }
  if (fs == 8000) { *r = {8000, 240, 60, 512, 10}; return true; }
  return false;
}

inline int64_t comp_frames(int64_t n, const CompRate& r) { return n > r.win ? (n - r.win) / r.skip : 0; }

struct CompLayout {
  int64_t P, fmax, fcap;
  int64_t off_stats, off_fr, off_sorted, total;
};

// 0: fine; 1: bad shape; 2: more frames than the ranking takes
int comp_layout(int B, int S, int64_t T, const CompRate& r, CompLayout* l) {
  if (B <= 0 || S < 1 || S > 3 || T < 1) return 1;
  if (T >= ((int64_t)1 << 31)) return 1;  // lengths are int32
  l->P = (int64_t)B * S;
  l->fmax = comp_frames(T, r);
  if (l->fmax > kMaxFrames) return 2;
  l->fcap = l->fmax > 0 ? l->fmax : 1;
  DsCarver ws;
  l->off_stats = ws.take(l->P * 4 * 8);
  l->off_fr = ws.take(l->P * 3 * l->fcap * 8);
  l->off_sorted = ws.take(l->P * 2 * l->fcap * 8);
  l->total = ws.total;
  return 0;
}

std::string comp_shape(int B, int S, int64_t T) {
  return "B=" + std::to_string(B) + " S=" + std::to_string(S) + " T=" + std::to_string(T);
}

// ---------------------------------------------------------------------------------------------------------------- tables
// Host side of the filter bank (evaluate_covl.py:235-246): weight of bin j in band i, exp(-11 ((j - floor(f0)) / bw)^2 +
// log(bw_min) - log(bandwidth)), zeroed at or below exp(-30 / (2 * 2.303)).  lo / hi: the non-zero bins [lo, hi) of a band;
// nb: one past the last bin any band reaches (the spectrum is computed for bins 0 .. nb - 1 only).
struct CompBands { int lo[kCrit], hi[kCrit], nb; };

void comp_filters(const CompRate& r, std::vector<double>* w, CompBands* bp) {
  const int half = r.nfft / 2;
  const double max_freq = r.fs / 2.0, min_factor = std::exp(-30.0 / (2.0 * 2.303));
  w->assign((size_t)kCrit * half, 0.0);
  bp->nb = 0;
  for (int i = 0; i < kCrit; ++i) {
    const double f0 = std::floor(kCent[i] / max_freq * half), bw = kBand[i] / max_freq * half;
    const double norm = std::log(kBand[0]) - std::log(kBand[i]);
    bp->lo[i] = half;
    bp->hi[i] = 0;
    for (int j = 0; j < half; ++j) {
      const double u = (j - f0) / bw, v = std::exp(-11.0 * (u * u) + norm);
      if (v > min_factor) {
        (*w)[(size_t)i * half + j] = v;
        if (j < bp->lo[i]) bp->lo[i] = j;
        bp->hi[i] = j + 1;
      }
    }
    if (bp->hi[i] < bp->lo[i]) bp->lo[i] = bp->hi[i] = 0;
    if (bp->hi[i] > bp->nb) bp->nb = bp->hi[i];
  }
}

// device doubles: window[kMaxWin] | cos(2 pi j / nfft), j < nfft, at kTabCos | sin(2 pi j / nfft) at kTabSin | filter weights
// [25][nb] at kTabFilt
constexpr int kTabWin = 0, kTabCos = kMaxWin, kTabSin = kMaxWin + kMaxFft, kTabFilt = kMaxWin + 2 * kMaxFft;

void comp_build_table(const CompRate& r, std::vector<double>& t, CompBands* bands) {
  const double pi = 3.14159265358979323846;
  std::vector<double> filt;
  comp_filters(r, &filt, bands);
  const int nb = bands->nb, half = r.nfft / 2;
  t.assign((size_t)kTabFilt + (size_t)kCrit * nb, 0.0);
  for (int j = 0; j < r.win; ++j) t[kTabWin + j] = 0.5 * (1.0 - std::cos(2.0 * pi * ((double)(j + 1) / (r.win + 1))));
  for (int j = 0; j < r.nfft; ++j) {
    t[kTabCos + j] = std::cos(2.0 * pi * j / r.nfft);
    t[kTabSin + j] = std::sin(2.0 * pi * j / r.nfft);
  }
  for (int i = 0; i < kCrit; ++i)
    for (int j = 0; j < nb; ++j) t[(size_t)kTabFilt + (size_t)i * nb + j] = filt[(size_t)i * half + j];
}

// ---------------------------------------------------------------------------------------------------------------- kernels
__device__ inline int comp_nframes(int len, int win, int skip) { return len > win ? (len - win) / skip : 0; }

// stats[pair][sig] = mean of the row over its len samples, stats[pair][2 + sig] = max |x - mean|.  grid (2, P), 256 threads
__global__ __launch_bounds__(256) void comp_stats_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                         const int* __restrict__ lengths, const int* __restrict__ perm,
                                                         double* __restrict__ stats, int S, long T) {
  __shared__ double sh4[4];
  const int pair = blockIdx.y, sig = blockIdx.x;
  const int len = ds_pair_len(lengths, pair / S, T);
  const float* x = ds_pair_row(ref, est, perm, pair, sig, S, T);
  double part = 0.0;
  for (int j = threadIdx.x; j < len; j += 256) part += (double)x[j];
  const double mean = ds_block_sum_d<4>(part, sh4) / (double)len;  // len = 0: NaN, and no frame reads it
  double mx = 0.0;
  for (int j = threadIdx.x; j < len; j += 256) mx = fmax(mx, fabs((double)x[j] - mean));
  mx = ds_block_max_d<4>(mx, sh4);
  if (threadIdx.x == 0) {
    stats[(long)pair * 4 + sig] = mean;
    stats[(long)pair * 4 + 2 + sig] = mx;
  }
}

struct CompFrameP { int win, skip, nfft, P; CompBands bands; };

// Levinson-Durbin in the reference's operation order (evaluate_covl.py:71-90) -> lp[0 .. P] = {1, -a}
__device__ inline void comp_lpc(const double* R, int P, double* lp) {
  double a[kMaxP], prev[kMaxP];
  double E = R[0];
  for (int i = 0; i < P; ++i) {
    double sum_term = 0.0;
    for (int j = 0; j < i; ++j) sum_term += a[j] * R[i - j];
    const double rc = (R[i + 1] - sum_term) / fmax(1e-15, E);
    for (int j = 0; j < i; ++j) prev[j] = a[j];
    for (int j = 0; j < i; ++j) a[j] = prev[j] - rc * prev[i - 1 - j];
    a[i] = rc;
    E = (1.0 - rc * rc) * E;
  }
  lp[0] = 1.0;
  for (int i = 0; i < P; ++i) lp[i + 1] = -a[i];
}

// a Toeplitz(R) a^T, rows in order
__device__ inline double comp_quad(const double* a, const double* R, int P) {
  double tot = 0.0;
  for (int i = 0; i <= P; ++i) {
    double row = 0.0;
    for (int j = 0; j <= P; ++j) row += R[i > j ? i - j : j - i] * a[j];
    tot += a[i] * row;
  }
  return tot;
}

// the peak of the spectrum nearest to band i in the direction of its slope (evaluate_covl.py:292-304, its comparisons and indices)
__device__ inline double comp_peak(const double* e, const double* slope, int i) {
  int n = i;
  if (slope[i] > 0) {
    while (n < kCrit - 1 && slope[n] > 0) ++n;
    return e[n - 1];
  }
  while (n >= 0 && slope[n] <= 0) --n;
  return e[n + 1];
}

// fr[pair][0 | 1 | 2][f] = LLR, WSS, segmental SNR of frame f (and frames_out [pair][3][frames_cap], nullable).
// grid (fcap, P), 256 threads
__global__ __launch_bounds__(256) void comp_frame_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                         const int* __restrict__ lengths, const int* __restrict__ perm,
                                                         const double* __restrict__ stats, const double* __restrict__ tab,
                                                         double* __restrict__ fr, double* __restrict__ frames_out,
                                                         long frames_cap, int S, long T, long fcap, CompFrameP p) {
  __shared__ double xw[2][kMaxWin];
  __shared__ double twc[kMaxFft], tws[kMaxFft];
  __shared__ double pw[2][kMaxFft / 2];
  __shared__ double R[2][kMaxP + 1], lp[2][kMaxP + 1];
  __shared__ double edb[2][kCrit], slope[2][kCrit - 1], peak[2][kCrit - 1];
  __shared__ double sh4[4];
  const int pair = blockIdx.y, f = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int len = ds_pair_len(lengths, pair / S, T);
  if (f >= comp_nframes(len, p.win, p.skip)) return;
  const float* x0 = ds_pair_row(ref, est, perm, pair, 0, S, T) + (long)f * p.skip;  // f skip + win <= len: inside the row
  const float* x1 = ds_pair_row(ref, est, perm, pair, 1, S, T) + (long)f * p.skip;
  const double mean0 = stats[(long)pair * 4], mean1 = stats[(long)pair * 4 + 1];
  const double scale = stats[(long)pair * 4 + 2] / stats[(long)pair * 4 + 3];
  double e_sig = 0.0, e_noise = 0.0;
  for (int j = t; j < p.win; j += 256) {
    const double w = tab[kTabWin + j], a = (double)x0[j], b = (double)x1[j];
    xw[0][j] = a * w;
    xw[1][j] = b * w;
    const double c = (a - mean0) * w, d = ((b - mean1) * scale) * w;
    e_sig += c * c;
    e_noise += (c - d) * (c - d);
  }
  for (int j = t; j < p.nfft; j += 256) {
    twc[j] = tab[kTabCos + j];
    tws[j] = tab[kTabSin + j];
  }
  e_sig = ds_block_sum_d<4>(e_sig, sh4);
  e_noise = ds_block_sum_d<4>(e_noise, sh4);  // (its barriers also publish xw and the twiddles)
  double segsnr = 10.0 * log10(e_sig / (e_noise + 1e-10) + 1e-10);
  segsnr = fmin(fmax(segsnr, -10.0), 35.0);

  // autocorrelation lags 0 .. P of both windowed frames: one (signal, lag) per wave at a time
  for (int idx = wave; idx < 2 * (p.P + 1); idx += 4) {
    const int sig = idx / (p.P + 1), k = idx % (p.P + 1);
    double part = 0.0;
    for (int j = lane; j < p.win - k; j += 64) part += xw[sig][j] * xw[sig][j + k];
    part = wave_sum_d(part);
    if (lane == 0) R[sig][k] = part;
  }
  // power spectrum of bins 0 .. nb - 1: X[k] = sum_j x[j] e^(-2 pi i j k / nfft), the twiddle index stepped by k modulo nfft
  for (int k = t; k < p.bands.nb; k += 256) {
    double re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
    int q = 0;
    for (int j = 0; j < p.win; ++j) {
      const double c = twc[q], s = tws[q], a = xw[0][j], b = xw[1][j];
      re0 += a * c;
      im0 -= a * s;
      re1 += b * c;
      im1 -= b * s;
      q = (q + k) & (p.nfft - 1);
    }
    pw[0][k] = re0 * re0 + im0 * im0;
    pw[1][k] = re1 * re1 + im1 * im1;
  }
  __syncthreads();
  if (t < 2) comp_lpc(R[t], p.P, lp[t]);
  if (t >= 64 && t < 64 + 2 * kCrit) {  // band energies in dB, floor 1e-10
    const int sig = (t - 64) / kCrit, band = (t - 64) % kCrit;
    const double* w = tab + kTabFilt + (long)band * p.bands.nb;
    double s = 0.0;
    for (int k = p.bands.lo[band]; k < p.bands.hi[band]; ++k) s += pw[sig][k] * w[k];
    edb[sig][band] = 10.0 * log10(fmax(s, 1e-10));
  }
  __syncthreads();
  if (t >= 64 && t < 64 + 2 * (kCrit - 1)) {
    const int sig = (t - 64) / (kCrit - 1), i = (t - 64) % (kCrit - 1);
    slope[sig][i] = edb[sig][i + 1] - edb[sig][i];
  }
  __syncthreads();
  if (t >= 64 && t < 64 + 2 * (kCrit - 1)) {
    const int sig = (t - 64) / (kCrit - 1), i = (t - 64) % (kCrit - 1);
    peak[sig][i] = comp_peak(edb[sig], slope[sig], i);
  }
  __syncthreads();
  if (t == 0) {
    const double num = fmax(1e-10, comp_quad(lp[1], R[0], p.P)), den = fmax(1e-10, comp_quad(lp[0], R[0], p.P));
    const double llr = log(num / den);
    double mx0 = edb[0][0], mx1 = edb[1][0];
    for (int i = 1; i < kCrit; ++i) { mx0 = fmax(mx0, edb[0][i]); mx1 = fmax(mx1, edb[1][i]); }
    double sw = 0.0, swd = 0.0;
    for (int i = 0; i < kCrit - 1; ++i) {
      const double w0 = (kKmax / (kKmax + mx0 - edb[0][i])) * (kKlocmax / (kKlocmax + peak[0][i] - edb[0][i]));
      const double w1 = (kKmax / (kKmax + mx1 - edb[1][i])) * (kKlocmax / (kKlocmax + peak[1][i] - edb[1][i]));
      const double w = (w0 + w1) / 2.0, d = slope[0][i] - slope[1][i];
      swd += w * (d * d);
      sw += w;
    }
    const double wss = swd / sw;
    double* o = fr + (long)pair * 3 * fcap + f;
    o[0] = llr;
    o[fcap] = wss;
    o[2 * fcap] = segsnr;
    if (frames_out) {
      double* fo = frames_out + (long)pair * 3 * frames_cap + f;
      fo[0] = llr;
      fo[frames_cap] = wss;
      fo[2 * frames_cap] = segsnr;
    }
  }
}

// a before b in the ranking: ascending, NaN last
__device__ inline bool comp_less(double a, double b) { return a < b || (a == a && b != b); }

// out[pair] = { mean of the m smallest LLRs, mean of the m smallest WSS values, mean segmental SNR, n }, m = rint(0.95 n).
// grid (P), 256 threads; sorted [P][2][fcap]
__global__ __launch_bounds__(256) void comp_final_kernel(const double* __restrict__ fr, const int* __restrict__ lengths,
                                                         double* __restrict__ sorted, double* __restrict__ out, int S, long T,
                                                         long fcap, int win, int skip) {
  __shared__ double tile[2][256];
  __shared__ double res[3];
  const int pair = blockIdx.x, t = threadIdx.x;
  const int n = comp_nframes(ds_pair_len(lengths, pair / S, T), win, skip);
  double* o = out + (long)pair * 4;
  if (n == 0) {
    if (t < 3) o[t] = __longlong_as_double(0x7ff8000000000000LL);
    if (t == 3) o[3] = 0.0;
    return;
  }
  const double* v0 = fr + (long)pair * 3 * fcap;
  const double* v1 = v0 + fcap;
  const double* v2 = v1 + fcap;
  double* s0 = sorted + (long)pair * 2 * fcap;
  double* s1 = s0 + fcap;
  // the rank of frame i = frames that sort before it (equal values: the earlier frame first), tile by tile through LDS
  for (int base = 0; base < n; base += 256) {
    const int i = base + t;
    const double a0 = i < n ? v0[i] : 0.0, a1 = i < n ? v1[i] : 0.0;
    int r0 = 0, r1 = 0;
    for (int jb = 0; jb < n; jb += 256) {
      __syncthreads();
      if (jb + t < n) { tile[0][t] = v0[jb + t]; tile[1][t] = v1[jb + t]; }
      __syncthreads();
      const int cnt = min(256, n - jb);
      for (int j = 0; j < cnt; ++j) {
        const double b0 = tile[0][j], b1 = tile[1][j];
        const bool first = jb + j < i;
        r0 += (comp_less(b0, a0) || (first && !comp_less(a0, b0))) ? 1 : 0;
        r1 += (comp_less(b1, a1) || (first && !comp_less(a1, b1))) ? 1 : 0;
      }
    }
    if (i < n) { s0[r0] = a0; s1[r1] = a1; }  // r < n: a permutation of 0 .. n - 1
  }
  __syncthreads();  // (block-wide visibility of the global writes above)
  const int m = (int)rint((double)n * 0.95);
  // sequential sums: thread 0 the m smallest LLRs ascending, thread 64 the same of WSS, thread 128 the segmental SNRs in frame order
  double acc = 0.0;
  for (int base = 0; base < n; base += 256) {
    __syncthreads();
    if (base + t < n) {
      tile[0][t] = s0[base + t];
      tile[1][t] = s1[base + t];
    }
    __syncthreads();
    if (t == 0 || t == 64) {
      const int cnt = min(256, m - base);
      for (int j = 0; j < cnt; ++j) acc += tile[t >> 6][j];
    }
    if (t == 128) {
      const int cnt = min(256, n - base);
      for (int j = 0; j < cnt; ++j) acc += v2[base + j];
    }
  }
  if (t == 0) res[0] = acc / (double)m;
  if (t == 64) res[1] = acc / (double)m;
  if (t == 128) res[2] = acc / (double)n;
  __syncthreads();
  if (t < 3) o[t] = res[t];
  if (t == 3) o[3] = (double)n;
}

}  // namespace

extern "C" int64_t diffsep_composite_workspace_bytes(int32_t B, int32_t S, int64_t T, int32_t fs) {
  CompRate r;
  CompLayout l;
  if (!comp_rate(fs, &r)) {
    ds_set_error("composite_workspace_bytes: unsupported sample rate " + std::to_string(fs) + " (16000 or 8000)");
    return -1;
  }
  const int rc = comp_layout(B, S, T, r, &l);
  if (rc == 1) {
    ds_set_error("composite_workspace_bytes: bad shape " + comp_shape(B, S, T) + " (B >= 1, S in 1..3, 1 <= T < 2^31)");
    return -1;
  }
  if (rc == 2) {
    ds_set_error("composite_workspace_bytes: " + std::to_string(comp_frames(T, r)) + " frames per row, the on-device ranking takes " +
                 std::to_string(kMaxFrames) + " (" + comp_shape(B, S, T) + ")");
    return -1;
  }
  return l.total;
}

extern "C" int32_t diffsep_composite(const float* ref, const float* est, double* out, double* frames_out, int64_t frames_cap,
                                     int32_t B, int32_t S, int64_t T, const int32_t* lengths, const int32_t* perm, int32_t fs,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  CompRate r;
  CompLayout l;
  DS_CHECK(comp_rate(fs, &r), "composite: unsupported sample rate " + std::to_string(fs) + " (16000 or 8000)");
  const int rc = comp_layout(B, S, T, r, &l);
  DS_CHECK(rc != 1, "composite: bad shape " + comp_shape(B, S, T));
  DS_CHECK(rc != 2, "composite: more than " + std::to_string(kMaxFrames) + " frames per row (" + comp_shape(B, S, T) + ")");
  DS_CHECK(!frames_out || frames_cap >= l.fmax, "composite: frames_cap " + std::to_string(frames_cap) + " < " +
                                                    std::to_string(l.fmax) + " frames of T");
  if (ds_pair_check("composite", ref, est, out, workspace, workspace_bytes, l.P, l.total)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const double* tab = nullptr;
  CompFrameP fp;
  if (ds_device_table({r.fs, 0}, [&](std::vector<double>& t, CompBands& b) { comp_build_table(r, t, &b); }, &tab, &fp.bands)) return 1;
  DS_CHECK(fp.bands.nb >= 1 && fp.bands.nb <= r.nfft / 2, "composite: filter bank outside the half spectrum");
  fp.win = r.win; fp.skip = r.skip; fp.nfft = r.nfft; fp.P = r.P;
  char* ws = (char*)workspace;
  double* stats = (double*)(ws + l.off_stats);
  double* fr = (double*)(ws + l.off_fr);
  double* sorted = (double*)(ws + l.off_sorted);
  const int P = (int)l.P;
  if (l.fmax > 0) {
    comp_stats_kernel<<<dim3(2, P), 256, 0, st>>>(ref, est, lengths, perm, stats, S, T);
    DS_LAUNCH_CHECK();
    comp_frame_kernel<<<dim3((unsigned)l.fmax, P), 256, 0, st>>>(ref, est, lengths, perm, stats, tab, fr, frames_out,
                                                                 frames_cap, S, T, l.fcap, fp);
    DS_LAUNCH_CHECK();
  }
  comp_final_kernel<<<P, 256, 0, st>>>(fr, lengths, sorted, out, S, T, l.fcap, r.win, r.skip);
  DS_LAUNCH_CHECK();
  return 0;
}
