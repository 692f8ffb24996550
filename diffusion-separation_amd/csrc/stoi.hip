// stoi.hip — STOI / ESTOI of a zero-padded batch on the device, float64 from the fp32 samples on.
//
// What the reference obtains from pystoi's stoi(ref, est, fs, extended) (evaluate.py:113-130), i.e. the algorithm of
//   C. H. Taal, R. C. Hendriks, R. Heusdens, J. Jensen, "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted
//   Noisy Speech", IEEE TASLP 19(7), 2011, and
//   J. Jensen, C. H. Taal, "An Algorithm for Predicting the Intelligibility of Speech Masked by Modulated Noise Maskers",
//   IEEE/ACM TASLP 24(11), 2016 (the extended measure),
// exactly as diffsep_amd/metrics.py and oracle/stoi_oracle.py state it: polyphase resampling to 10 kHz, removal of the frames
// whose clean energy lies 40 dB below the loudest one, 15 one-third octave bands of 256-sample Hann frames (512-point DFT),
// 30-frame segments.
//
// One pair = (utterance b, reference row i, estimate row perm[b][i]).  Launch sequence (grid over pairs x samples / frames /
// segments; no host loop over utterances, no readback: the kept-frame count stays on the device):
//   stoi_resample_kernel  fp32 rows -> float64 at 10 kHz (taps from a host-built float64 table; fs = 10 kHz: a cast)
//   stoi_energy_kernel    dB energy of every windowed reference frame
//   stoi_keep_kernel      per pair: loudest frame, keep mask, prefix sum -> list of kept frames + their number
//   stoi_bands_kernel     per frame of the compacted signals (overlap-added on the fly from the kept frames): a 512-point
//                         radix-2 FFT in LDS of each of the two signals (twiddles from the host-built float64 table; one FFT
//                         of ref + i est would leak the louder signal's rounding into the other: an all-zero reference must
//                         give exactly zero bands), power summed over the bins of each band, sqrt
//   stoi_segment_kernel   per 30-frame segment: the ESTOI / STOI term
//   stoi_final_kernel     per pair: sum over segments in a fixed order, the 1e-5 sentinel below 30 frames
// Every reduction has a fixed order that depends on the pair's own length only (reduce_device.h; no floating-point atomics):
// row (b, i) of a batch equals the B = 1 call bit for bit, on any stream.  Pair addressing, workspace carving, the table cache
// and the boundary checks are those of every measure on pairs: pair_metrics.h.
#include <cmath>

#include "../../include/diffsep_hip.h"
#include "common.h"
#include "pair_metrics.h"
#include "reduce_device.h"
#include "resample_design.h"

namespace {

constexpr int kFs = 10000, kNw = 256, kHop = 128, kNfft = 512, kBands = 15, kSeg = 30;
constexpr double kDyn = 40.0, kEps = 2.220446049250313e-16;  // np.finfo(float64).eps
constexpr int kMaxRatio = kResampleMaxRatio;  // largest p or q of the reduced 10000 / fs the tap table is built for

struct Ratio { int p, q, L; };

// p / q = 10000 / fs reduced; L = half-length of the anti-aliasing filter (Octave's resample design, 60 dB)
bool stoi_ratio(int fs, Ratio* r) {
  if (fs <= 0) return false;
  int a = kFs, b = fs;
  while (b) { int t = a % b; a = b; b = t; }
  r->p = kFs / a;
  r->q = fs / a;
  if ((r->p > r->q ? r->p : r->q) > kMaxRatio) return false;
  r->L = ds_resample_half_length(r->p, r->q);
  return true;
}

inline int64_t stoi_frames(int64_t n) { return n > kNw ? (n - kNw + kHop - 1) / kHop : 0; }  // len(range(0, n - 256, 128))

// band edges in DFT bins (band_edges() of the oracle): [a, b) per band, the bin nearest to 150 * 2^((2k -+ 1) / 6) Hz
void stoi_band_edges(int* lo, int* hi) {
  for (int k = 0; k < kBands; ++k) {
    const double fl = 150.0 * std::pow(2.0, (2 * k - 1) / 6.0), fh = 150.0 * std::pow(2.0, (2 * k + 1) / 6.0);
    int a = 0, b = 0;
    double da = 1e300, db = 1e300;
    for (int i = 0; i <= kNfft / 2; ++i) {  // first minimum, like argmin
      const double f = (double)kFs * i / kNfft;
      if ((f - fl) * (f - fl) < da) { da = (f - fl) * (f - fl); a = i; }
      if ((f - fh) * (f - fh) < db) { db = (f - fh) * (f - fh); b = i; }
    }
    lo[k] = a;
    hi[k] = b;
  }
}

struct StoiLayout {
  int64_t P, nmax, fmax;
  int64_t off_xr, off_energy, off_kidx, off_nkeep, off_bands, off_seg, total;
};

bool stoi_layout(int B, int S, int64_t T, const Ratio& r, StoiLayout* l) {
  if (B <= 0 || S <= 0 || T <= 0) return false;
  if (T >= ((int64_t)1 << 31)) return false;  // lengths are int32
  l->P = (int64_t)B * S;
  l->nmax = (T * r.p + r.q - 1) / r.q;
  if (l->nmax >= ((int64_t)1 << 31) - 4096) return false;
  l->fmax = stoi_frames(l->nmax);
  const int64_t fm = l->fmax > 0 ? l->fmax : 1;
  DsCarver ws;
  l->off_xr = ws.take(l->P * 2 * l->nmax * 8);
  l->off_energy = ws.take(l->P * fm * 8);
  l->off_kidx = ws.take(l->P * fm * 4);
  l->off_nkeep = ws.take(l->P * 4);
  l->off_bands = ws.take(l->P * 2 * fm * kBands * 8);
  l->off_seg = ws.take(l->P * fm * 8);
  l->total = ws.total;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- tables
// device doubles: hann[256] | cos(2 pi j / 512), j < 256 | -sin(2 pi j / 512), j < 256 | taps h[2 L + 1] (scaled by p)
constexpr int kTabHann = 0, kTabCos = 256, kTabSin = 512, kTabTaps = 768;

void stoi_build_table(const Ratio& r, std::vector<double>& t) {
  const double pi = 3.14159265358979323846;
  t.assign(kTabTaps + 2 * r.L + 1, 0.0);
  for (int k = 0; k < kNw; ++k) t[kTabHann + k] = 0.5 * (1.0 - std::cos(2.0 * pi * (k + 1) / (kNw + 1)));  // Matlab hanning(256)
  for (int j = 0; j < kNfft / 2; ++j) {
    t[kTabCos + j] = std::cos(2.0 * pi * j / kNfft);
    t[kTabSin + j] = -std::sin(2.0 * pi * j / kNfft);
  }
  ds_resample_design(r.p, r.q, r.L, &t[kTabTaps]);  // Kaiser-windowed sinc, unit DC gain after the zero stuffing
}

struct StoiBandsP { int lo[kBands], hi[kBands]; };

// ---------------------------------------------------------------------------------------------------------------- kernels
__device__ inline long stoi_nout(int len, int p, int q) { return ((long)len * p + q - 1) / q; }
__device__ inline int stoi_nframes(long n) { return n > kNw ? (int)((n - kNw + kHop - 1) / kHop) : 0; }

// y[m] = sum_j h[m q + L - p j] x[j]: the zero-stuffed direct form, centred, n_out = ceil(len p / q).
// grid (ceil(nmax / 256), 2, P); xr [P][2][nmax]
__global__ __launch_bounds__(256) void stoi_resample_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                            const int* __restrict__ lengths, const int* __restrict__ perm,
                                                            const double* __restrict__ taps, double* __restrict__ xr, int S,
                                                            long T, long nmax, int p, int q, int L) {
  const int pair = blockIdx.z, sig = blockIdx.y;
  const int len = ds_pair_len(lengths, pair / S, T);
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= stoi_nout(len, p, q)) return;
  const float* x = ds_pair_row(ref, est, perm, pair, sig, S, T);
  const long c = m * q + L, a = c - 2 * (long)L;
  long jlo = a > 0 ? (a + p - 1) / p : 0, jhi = c / p;
  if (jhi > len - 1) jhi = len - 1;
  double acc = 0.0;
  for (long j = jlo; j <= jhi; ++j) acc += taps[c - p * j] * (double)x[j];
  xr[((long)pair * 2 + sig) * nmax + m] = acc;
}

// energy[pair][f] = 20 log10(|w x_ref[128 f .. 128 f + 256)| + eps).  grid (fcap, P)
__global__ __launch_bounds__(256) void stoi_energy_kernel(const double* __restrict__ xr, const int* __restrict__ lengths,
                                                          const double* __restrict__ tab, double* __restrict__ energy, int S,
                                                          long T, long nmax, long fcap, int p, int q) {
  __shared__ double sh4[4];
  const int pair = blockIdx.y, f = blockIdx.x;
  const int nfr = stoi_nframes(stoi_nout(ds_pair_len(lengths, pair / S, T), p, q));
  if (f >= nfr) return;
  const double v = tab[kTabHann + threadIdx.x] * xr[(long)pair * 2 * nmax + (long)f * kHop + threadIdx.x];
  const double s = ds_block_sum_d<4>(v * v, sh4);
  if (threadIdx.x == 0) energy[(long)pair * fcap + f] = 20.0 * log10(sqrt(s) + kEps);
}

// kidx[pair][0 .. nkeep) = the frames with max(e) - 40 - e < 0, ascending.  grid (P), 256 threads, each a contiguous chunk.
__global__ __launch_bounds__(256) void stoi_keep_kernel(const double* __restrict__ energy, const int* __restrict__ lengths,
                                                        int* __restrict__ kidx, int* __restrict__ nkeep, int S, long T,
                                                        long fcap, int p, int q) {
  __shared__ double shmax[256];
  __shared__ int shcnt[256];
  const int pair = blockIdx.x, t = threadIdx.x;
  const int nfr = stoi_nframes(stoi_nout(ds_pair_len(lengths, pair / S, T), p, q));
  const double* e = energy + (long)pair * fcap;
  const int chunk = (nfr + 255) / 256, f0 = t * chunk, f1 = min(nfr, f0 + chunk);
  double mx = -1e300;
  for (int f = f0; f < f1; ++f) mx = fmax(mx, e[f]);
  shmax[t] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) shmax[t] = fmax(shmax[t], shmax[t + o]);
    __syncthreads();
  }
  mx = shmax[0];
  int cnt = 0;
  for (int f = f0; f < f1; ++f) cnt += (mx - kDyn - e[f] < 0.0) ? 1 : 0;
  shcnt[t] = cnt;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < 256; ++k) { const int c = shcnt[k]; shcnt[k] = run; run += c; }
    nkeep[pair] = run;
  }
  __syncthreads();
  int o = shcnt[t];
  for (int f = f0; f < f1; ++f)
    if (mx - kDyn - e[f] < 0.0) kidx[(long)pair * fcap + o++] = f;
}

// Frame m of the compacted signals: sample 128 m + t lies in the kept frames a = m + (t >= 128) and a - 1 (overlap-add of the
// windowed kept frames, the earlier one first), windowed again, 512-point FFT of each signal, one-third octave band magnitudes.
// grid (fcap, P), 256 threads; bands [P][2][fcap][15]
__global__ __launch_bounds__(256) void stoi_bands_kernel(const double* __restrict__ xr, const int* __restrict__ kidx,
                                                         const int* __restrict__ nkeep, const double* __restrict__ tab,
                                                         double* __restrict__ bands, long nmax, long fcap, StoiBandsP bp) {
  __shared__ double zr[2][kNfft], zi[2][kNfft];
  __shared__ double pw[2][kNfft / 2];
  const int pair = blockIdx.y, m = blockIdx.x, t = threadIdx.x;
  const int nk = nkeep[pair];
  if (m >= nk - 1) return;  // (nk + 1) * 128 compacted samples hold nk - 1 frames (the authors' strict loop bound)
  {
    const double* x0 = xr + (long)pair * 2 * nmax;
    const double* x1 = x0 + nmax;
    const int* kd = kidx + (long)pair * fcap;
    const int a = m + (t >> 7), u = t & 127;  // sample = 128 a + u: offset u + 128 in kept frame a - 1, offset u in kept frame a
    double vr = 0.0, vi = 0.0;
    if (a >= 1) {
      const long s = (long)kd[a - 1] * kHop + u + kHop;
      const double w = tab[kTabHann + u + kHop];
      vr = w * x0[s];
      vi = w * x1[s];
    }
    if (a < nk) {
      const long s = (long)kd[a] * kHop + u;
      const double w = tab[kTabHann + u];
      vr += w * x0[s];
      vi += w * x1[s];
    }
    const double w = tab[kTabHann + t];
    zr[0][t] = w * vr;
    zr[1][t] = w * vi;
    zi[0][t] = zi[1][t] = 0.0;
    zr[0][t + 256] = zr[1][t + 256] = zi[0][t + 256] = zi[1][t + 256] = 0.0;
  }
  __syncthreads();
  // decimation in frequency, natural order in, bit-reversed order out: one butterfly per thread and stage
  for (int h = 256, sh = 0; h >= 1; h >>= 1, ++sh) {
    const int j = t & (h - 1), i0 = ((t - j) << 1) + j, i1 = i0 + h;
    const double wr = tab[kTabCos + (j << sh)], wi = tab[kTabSin + (j << sh)];
#pragma unroll
    for (int sig = 0; sig < 2; ++sig) {
      const double ar = zr[sig][i0], ai = zi[sig][i0], br = zr[sig][i1], bi = zi[sig][i1];
      const double dr = ar - br, di = ai - bi;
      zr[sig][i0] = ar + br;
      zi[sig][i0] = ai + bi;
      zr[sig][i1] = dr * wr - di * wi;
      zi[sig][i1] = dr * wi + di * wr;
    }
    __syncthreads();
  }
  {  // bin k of the real signals' spectra sits at the bit-reversed index
    const int rk = (int)(__brev((unsigned)t) >> 23);
    pw[0][t] = zr[0][rk] * zr[0][rk] + zi[0][rk] * zi[0][rk];
    pw[1][t] = zr[1][rk] * zr[1][rk] + zi[1][rk] * zi[1][rk];
  }
  __syncthreads();
  if (t < 2 * kBands) {
    const int sig = t / kBands, band = t % kBands;
    double s = 0.0;
    for (int k = bp.lo[band]; k < bp.hi[band]; ++k) s += pw[sig][k];
    bands[(((long)pair * 2 + sig) * fcap + m) * kBands + band] = sqrt(s);
  }
}

// segval[pair][g] = the term of segment g (frames g .. g + 29): ESTOI sum of products / 30 of the row- then column-normalised
// segments; STOI the sum over bands of the clipped, zero-mean correlation.  grid (fcap, P), 64 threads
__global__ __launch_bounds__(64) void stoi_segment_kernel(const double* __restrict__ bands, const int* __restrict__ nkeep,
                                                          double* __restrict__ segval, long fcap, int extended) {
  __shared__ double sx[2][kBands][kSeg + 1];
  const int pair = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
  const int M = nkeep[pair] - 1;
  if (g + kSeg > M) return;
  for (int e = t; e < 2 * kBands * kSeg; e += 64) {
    const int sig = e / (kBands * kSeg), r = e % (kBands * kSeg), n = r / kBands, j = r % kBands;
    sx[sig][j][n] = bands[(((long)pair * 2 + sig) * fcap + g + n) * kBands + j];
  }
  __syncthreads();
  double term = 0.0;
  if (extended) {
    if (t < 2 * kBands) {  // rows (bands) to zero mean / unit norm
      double* a = sx[t / kBands][t % kBands];
      double mu = 0.0, ss = 0.0;
      for (int n = 0; n < kSeg; ++n) mu += a[n];
      mu /= kSeg;
      for (int n = 0; n < kSeg; ++n) { a[n] -= mu; ss += a[n] * a[n]; }
      const double d = sqrt(ss) + kEps;
      for (int n = 0; n < kSeg; ++n) a[n] /= d;
    }
    __syncthreads();
    if (t < 2 * kSeg) {  // columns (frames)
      const int sig = t / kSeg, n = t % kSeg;
      double mu = 0.0, ss = 0.0;
      for (int j = 0; j < kBands; ++j) mu += sx[sig][j][n];
      mu /= kBands;
      for (int j = 0; j < kBands; ++j) { const double v = sx[sig][j][n] - mu; sx[sig][j][n] = v; ss += v * v; }
      const double d = sqrt(ss) + kEps;
      for (int j = 0; j < kBands; ++j) sx[sig][j][n] /= d;
    }
    __syncthreads();
    double part = 0.0;
    if (t < kSeg)
      for (int j = 0; j < kBands; ++j) part += sx[0][j][t] * sx[1][j][t];
    term = wave_sum_d(part) / kSeg;
  } else {
    double part = 0.0;
    if (t < kBands) {
      const double* x = sx[0][t];
      const double* y = sx[1][t];
      const double clip = 1.0 + 5.623413251903491;  // 1 + 10^(15 / 20)
      double nx = 0.0, ny = 0.0;
      for (int n = 0; n < kSeg; ++n) { nx += x[n] * x[n]; ny += y[n] * y[n]; }
      const double alpha = sqrt(nx) / (sqrt(ny) + kEps);
      double mx = 0.0, my = 0.0;
      for (int n = 0; n < kSeg; ++n) { mx += x[n]; my += fmin(alpha * y[n], clip * x[n]); }
      mx /= kSeg;
      my /= kSeg;
      double sxx = 0.0, syy = 0.0, sxy = 0.0;
      for (int n = 0; n < kSeg; ++n) {
        const double xc = x[n] - mx, yc = fmin(alpha * y[n], clip * x[n]) - my;
        sxx += xc * xc; syy += yc * yc; sxy += xc * yc;
      }
      part = sxy / ((sqrt(sxx) + kEps) * (sqrt(syy) + kEps));
    }
    term = wave_sum_d(part);
  }
  if (t == 0) segval[(long)pair * fcap + g] = term;
}

// out[pair] = mean over segments (and bands for STOI); fewer than 30 frames: 1e-5.  grid (P), 256 threads
__global__ __launch_bounds__(256) void stoi_final_kernel(const double* __restrict__ segval, const int* __restrict__ nkeep,
                                                         double* __restrict__ out, long fcap, int extended) {
  __shared__ double sh4[4];
  const int pair = blockIdx.x;
  const int M = nkeep[pair] - 1;
  if (M < kSeg) {
    if (threadIdx.x == 0) out[pair] = 1e-5;
    return;
  }
  const int nseg = M - kSeg + 1;
  double part = 0.0;
  for (int g = threadIdx.x; g < nseg; g += 256) part += segval[(long)pair * fcap + g];
  const double s = ds_block_sum_d<4>(part, sh4);
  if (threadIdx.x == 0) out[pair] = extended ? s / nseg : s / ((double)nseg * kBands);
}

}  // namespace

extern "C" int64_t diffsep_stoi_workspace_bytes(int32_t B, int32_t S, int64_t T, int32_t fs) {
  Ratio r;
  StoiLayout l;
  if (!stoi_ratio(fs, &r)) {
    ds_set_error("stoi_workspace_bytes: unsupported sample rate " + std::to_string(fs) + " (10000 / fs must reduce to p / q <= " +
                 std::to_string(kMaxRatio) + ")");
    return -1;
  }
  if (!stoi_layout(B, S, T, r, &l)) {
    ds_set_error("stoi_workspace_bytes: bad shape B=" + std::to_string(B) + " S=" + std::to_string(S) + " T=" + std::to_string(T));
    return -1;
  }
  return l.total;
}

extern "C" int32_t diffsep_stoi(const float* ref, const float* est, double* out, int32_t B, int32_t S, int64_t T,
                                const int32_t* lengths, const int32_t* perm, int32_t fs, int32_t extended, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  Ratio r;
  StoiLayout l;
  DS_CHECK(stoi_ratio(fs, &r), "stoi: unsupported sample rate " + std::to_string(fs));
  DS_CHECK(stoi_layout(B, S, T, r, &l), "stoi: bad shape B=" + std::to_string(B) + " S=" + std::to_string(S) + " T=" + std::to_string(T));
  if (ds_pair_check("stoi", ref, est, out, workspace, workspace_bytes, l.P, l.total)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const double* tab = nullptr;
  DsNoExtra none;
  if (ds_device_table({r.p, r.q}, [&](std::vector<double>& t, DsNoExtra&) { stoi_build_table(r, t); }, &tab, &none)) return 1;
  char* ws = (char*)workspace;
  double* xr = (double*)(ws + l.off_xr);
  double* energy = (double*)(ws + l.off_energy);
  int* kidx = (int*)(ws + l.off_kidx);
  int* nkeep = (int*)(ws + l.off_nkeep);
  double* bands = (double*)(ws + l.off_bands);
  double* segval = (double*)(ws + l.off_seg);
  const int P = (int)l.P;
  StoiBandsP bp;
  stoi_band_edges(bp.lo, bp.hi);
  stoi_resample_kernel<<<dim3(cdiv(l.nmax, 256), 2, P), 256, 0, st>>>(ref, est, lengths, perm, tab + kTabTaps, xr, S, T, l.nmax,
                                                                      r.p, r.q, r.L);
  DS_LAUNCH_CHECK();
  if (l.fmax > 0) {
    stoi_energy_kernel<<<dim3((unsigned)l.fmax, P), 256, 0, st>>>(xr, lengths, tab, energy, S, T, l.nmax, l.fmax, r.p, r.q);
    DS_LAUNCH_CHECK();
  }
  stoi_keep_kernel<<<P, 256, 0, st>>>(energy, lengths, kidx, nkeep, S, T, l.fmax, r.p, r.q);
  DS_LAUNCH_CHECK();
  if (l.fmax > 1) {
    stoi_bands_kernel<<<dim3((unsigned)l.fmax - 1, P), 256, 0, st>>>(xr, kidx, nkeep, tab, bands, l.nmax, l.fmax, bp);
    DS_LAUNCH_CHECK();
  }
  if (l.fmax > kSeg) {
    stoi_segment_kernel<<<dim3((unsigned)l.fmax - kSeg, P), 64, 0, st>>>(bands, nkeep, segval, l.fmax, extended ? 1 : 0);
    DS_LAUNCH_CHECK();
  }
  stoi_final_kernel<<<P, 256, 0, st>>>(segval, nkeep, out, l.fmax, extended ? 1 : 0);
  DS_LAUNCH_CHECK();
  return 0;
}
