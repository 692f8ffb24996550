// resample.hip — band-limited sample-rate conversion of fp32 rows on the device, by any reduced ratio p / q with an odd-length FIR.
//
// Definition (the zero-stuffed direct form, centred; what scipy.signal.resample_poly(x, p, q, window=h / p) computes and what
// stoi_resample_kernel computes): with taps h[0 .. 2 L] in float64 and a row x[0 .. len) of fp32 samples,
//   y[m] = sum_j h[m q + L - p j] (double)x[j],   0 <= j < len, tap index in [0, 2 L],   0 <= m < n_out = ceil(len p / q).
// Float64 throughout, each term entering by ONE fused multiply-add (acc = fma(h, x, acc): the product is not rounded on its own, so
// an unfused float64 reference agrees within the summation bound, not bit for bit, unless every sum is exact); one rounding at the
// end for fp32 output.
//
// Polyphase form: with c = m q + L, j0 = c div p and phase = c mod p the terms are h[phase + p k] x[j0 - k], k = 0 .. K - 1,
// K = ceil((2 L + 1) / p).  phase depends on r = m mod p only, so the table is stored on the device as tab[k][r] = h[phase(r) + p k]
// (zero where the index passes 2 L): the lanes of a wave, consecutive m, read consecutive doubles of one table row for every k.
// Each output is the sum over k ascending, started from +0: a fixed order that depends on p, q and L only (terms outside the row
// are exact zeros and change nothing), no atomics: a row comes out bit for bit the same alone, inside any batch, on any stream.
//
//   resample_tile_kernel  one block = 256 consecutive outputs of one row; the input span of the tile (its 255 q / p + K samples,
//                         zero outside the row) is staged through LDS once, then every thread walks its K taps.  Taps: p = 1, one
//                         row for every lane, uniform (scalar) loads; a table of up to 2048 doubles (2:1, 3:2, 6:1 ...) is staged
//                         in LDS beside the samples; larger ones (the 441-based ratios: 32 K doubles) are read from L2, coalesced
//   resample_gather_kernel  the same sums with x gathered from global memory: ratios whose tile span does not fit in LDS
//                         (span = 255 q / p + K + 1 > 16000 floats: q / p from 49 on with the designed filters, whose K grows with
//                         q — 48 is the last that fits —, from 63 on with a short caller-supplied FIR)
// Columns [n_out of the row, ceil(T p / q)) are written as zeros: the result is a valid zero-padded batch.
#include <vector>

#include "../../include/diffsep_hip.h"
#include "common.h"
#include "resample_design.h"

struct diffsep_resampler {
  int p, q, L, K;
  int device;
  long span;      // floats of LDS of one tile; 0: the gather kernel
  bool tab_lds;   // the tile kernel stages the tap table in LDS too
  double* tab;    // [K][p] on `device`
};

namespace {

constexpr int kTile = 256;              // outputs per block = threads per block
constexpr long kSpanMax = 16000;        // floats: 64 KB of LDS per block at most
constexpr int kMaxTaps = 1 << 17;
constexpr int kTabLdsMax = 2048;        // doubles: a tap table up to this size is staged in LDS (with the span: 64 KB at most)
enum { kTapsUniform, kTapsLds, kTapsGlobal };  // where the tile kernel reads its taps from

template <typename Out> struct OutT;
template <> struct OutT<float> { __device__ static inline float of(double v) { return (float)v; } };
template <> struct OutT<double> { __device__ static inline double of(double v) { return v; } };

__device__ inline long rs_len(const int* lengths, long row, int rpl, long T) {
  long n = lengths ? (long)lengths[row / rpl] : T;
  return n < 0 ? 0 : (n > T ? T : n);
}
__device__ inline long rs_nout(long len, int p, int q) { return (len * p + q - 1) / q; }

// grid (tiles, rows); dynamic LDS: span floats (rounded up to an even number), then K p doubles with kTapsLds
template <typename Out, int Taps>
__global__ __launch_bounds__(kTile) void resample_tile_kernel(const float* __restrict__ x, long ldx, Out* __restrict__ y, long ldy,
                                                              long T, long nmax, const int* __restrict__ lengths, int rpl,
                                                              int* __restrict__ lengths_out, const double* __restrict__ tab,
                                                              int p, int q, int L, int K, int span) {
  extern __shared__ float sx[];
  const long row = blockIdx.y;
  const long len = rs_len(lengths, row, rpl, T), nout = rs_nout(len, p, q);
  const long m0 = (long)blockIdx.x * kTile, m = m0 + threadIdx.x;
  if (lengths_out && blockIdx.x == 0 && threadIdx.x == 0 && row % rpl == 0) lengths_out[row / rpl] = (int)nout;
  Out* yr = y + row * ldy;
  if (m0 >= nout) {  // the whole tile lies in the zero padding
    if (m < nmax) yr[m] = OutT<Out>::of(0.0);
    return;
  }
  const float* xr = x + row * ldx;
  const long jbase = (m0 * q + L) / p - (K - 1);
  for (int i = threadIdx.x; i < span; i += kTile) {
    const long j = jbase + i;
    sx[i] = (j >= 0 && j < len) ? xr[j] : 0.0f;
  }
  double* stab = reinterpret_cast<double*>(sx + ((span + 1) & ~1));
  if (Taps == kTapsLds)
    for (int i = threadIdx.x; i < K * p; i += kTile) stab[i] = tab[i];
  __syncthreads();
  if (m >= nmax) return;
  double acc = 0.0;
  if (m < nout) {
    const long c = m * q + L;
    const int off = (int)(c / p - jbase);  // LDS index of x[j0]; in [K - 1, span)
    if (Taps == kTapsLds) {
      const double* t = stab + (m % p);
#pragma unroll 4
      for (int k = 0; k < K; ++k) acc += t[k * p] * (double)sx[off - k];
    } else {
      const double* t = Taps == kTapsUniform ? tab : tab + (m % p);
#pragma unroll 4
      for (int k = 0; k < K; ++k) acc += t[(long)k * p] * (double)sx[off - k];
    }
  }
  yr[m] = OutT<Out>::of(acc);
}

// grid (tiles, rows): one thread per output, x straight from global memory
template <typename Out>
__global__ __launch_bounds__(kTile) void resample_gather_kernel(const float* __restrict__ x, long ldx, Out* __restrict__ y, long ldy,
                                                                long T, long nmax, const int* __restrict__ lengths, int rpl,
                                                                int* __restrict__ lengths_out, const double* __restrict__ tab,
                                                                int p, int q, int L, int K) {
  const long row = blockIdx.y;
  const long len = rs_len(lengths, row, rpl, T), nout = rs_nout(len, p, q);
  const long m = (long)blockIdx.x * kTile + threadIdx.x;
  if (lengths_out && blockIdx.x == 0 && threadIdx.x == 0 && row % rpl == 0) lengths_out[row / rpl] = (int)nout;
  if (m >= nmax) return;
  double acc = 0.0;
  if (m < nout) {
    const float* xr = x + row * ldx;
    const long c = m * q + L, j0 = c / p;
    const double* t = tab + (m % p);
    // (k outside [klo, khi] meets samples outside the row: exact zeros in the tile kernel, skipped here)
    const long klo = j0 > len - 1 ? j0 - (len - 1) : 0, khi = j0 < K - 1 ? j0 : K - 1;
    for (long k = klo; k <= khi; ++k) acc += t[k * p] * (double)xr[j0 - k];
  }
  y[row * ldy + m] = OutT<Out>::of(acc);
}

int rs_gcd(int a, int b) {
  while (b) { int t = a % b; a = b; b = t; }
  return a;
}

template <typename Out>
int rs_launch(const diffsep_resampler* r, const float* x, long ldx, void* y, long ldy, int rows, long T, long nmax,
              const int* lengths, int rpl, int* lengths_out, hipStream_t st) {
  const dim3 grid((unsigned)((nmax + kTile - 1) / kTile), (unsigned)rows);
  if (r->span == 0) {
    resample_gather_kernel<Out><<<grid, kTile, 0, st>>>(x, ldx, (Out*)y, ldy, T, nmax, lengths, rpl, lengths_out, r->tab, r->p, r->q,
                                                        r->L, r->K);
  } else if (r->p == 1) {
    resample_tile_kernel<Out, kTapsUniform><<<grid, kTile, r->span * sizeof(float), st>>>(
        x, ldx, (Out*)y, ldy, T, nmax, lengths, rpl, lengths_out, r->tab, r->p, r->q, r->L, r->K, (int)r->span);
  } else if (r->tab_lds) {
    const size_t lds = ((r->span + 1) & ~1L) * sizeof(float) + (size_t)r->K * r->p * sizeof(double);
    resample_tile_kernel<Out, kTapsLds><<<grid, kTile, lds, st>>>(x, ldx, (Out*)y, ldy, T, nmax, lengths, rpl, lengths_out, r->tab, r->p,
                                                                  r->q, r->L, r->K, (int)r->span);
  } else {
    resample_tile_kernel<Out, kTapsGlobal><<<grid, kTile, r->span * sizeof(float), st>>>(
        x, ldx, (Out*)y, ldy, T, nmax, lengths, rpl, lengths_out, r->tab, r->p, r->q, r->L, r->K, (int)r->span);
  }
  DS_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int32_t diffsep_resample_ratio(int32_t fs_in, int32_t fs_out, int32_t* p, int32_t* q) {
  DS_CHECK(p && q, "resample_ratio: null pointer");
  DS_CHECK(fs_in > 0 && fs_out > 0, "resample_ratio: sample rates must be positive (" + std::to_string(fs_in) + " -> " +
                                        std::to_string(fs_out) + ")");
  const int g = rs_gcd(fs_out, fs_in);
  const int pp = fs_out / g, qq = fs_in / g;
  DS_CHECK(pp <= kResampleMaxRatio && qq <= kResampleMaxRatio,
           "resample_ratio: " + std::to_string(fs_in) + " -> " + std::to_string(fs_out) + " Hz reduces to " + std::to_string(pp) + " / " +
               std::to_string(qq) + ", beyond the largest supported factor " + std::to_string(kResampleMaxRatio));
  *p = pp;
  *q = qq;
  return 0;
}

extern "C" int64_t diffsep_resample_length(int64_t n, int32_t p, int32_t q) {
  if (n < 0 || p <= 0 || q <= 0) {
    ds_set_error("resample_length: n >= 0 and p, q >= 1 expected (n=" + std::to_string(n) + " p=" + std::to_string(p) + " q=" +
                 std::to_string(q) + ")");
    return -1;
  }
  if (n > (INT64_MAX - q) / p) {
    ds_set_error("resample_length: n p does not fit in 64 bits (n=" + std::to_string(n) + " p=" + std::to_string(p) + ")");
    return -1;
  }
  return (n * p + q - 1) / q;
}

extern "C" int32_t diffsep_resample_design(int32_t p, int32_t q, double* taps_out, int32_t cap) {
  if (p <= 0 || q <= 0 || p > kResampleMaxRatio || q > kResampleMaxRatio || rs_gcd(p, q) != 1) {
    ds_set_error("resample_design: p / q = " + std::to_string(p) + " / " + std::to_string(q) + " must be reduced, with 1 <= p, q <= " +
                 std::to_string(kResampleMaxRatio));
    return -1;
  }
  const int L = ds_resample_half_length(p, q), n = 2 * L + 1;
  if (!taps_out) return n;
  if (cap < n) {
    ds_set_error("resample_design: " + std::to_string(n) + " taps do not fit in " + std::to_string(cap));
    return -1;
  }
  ds_resample_design(p, q, L, taps_out);
  return n;
}

extern "C" int32_t diffsep_resampler_create(int32_t p, int32_t q, const double* taps, int32_t ntaps, diffsep_resampler** out) {
  DS_CHECK(out, "resampler_create: null pointer");
  *out = nullptr;
  DS_CHECK(taps, "resampler_create: null taps");
  DS_CHECK(ntaps > 0 && ntaps % 2 == 1, "resampler_create: the number of taps must be odd and positive (" + std::to_string(ntaps) + ")");
  DS_CHECK(ntaps <= kMaxTaps, "resampler_create: more than " + std::to_string(kMaxTaps) + " taps (" + std::to_string(ntaps) + ")");
  DS_CHECK(p >= 1 && q >= 1 && p <= kResampleMaxRatio && q <= kResampleMaxRatio && rs_gcd(p, q) == 1,
           "resampler_create: p / q = " + std::to_string(p) + " / " + std::to_string(q) + " must be reduced, with 1 <= p, q <= " +
               std::to_string(kResampleMaxRatio));
  diffsep_resampler r{};
  r.p = p;
  r.q = q;
  r.L = (ntaps - 1) / 2;
  r.K = (ntaps + p - 1) / p;
  const long span = ((long)(kTile - 1) * q + p - 1) / p + r.K + 1;
  r.span = span <= kSpanMax ? span : 0;
  r.tab_lds = r.span && p > 1 && (long)r.K * p <= kTabLdsMax && ((span + 1) & ~1L) * 4 + (long)r.K * p * 8 <= 65536;
  std::vector<double> t((size_t)r.K * p, 0.0);
  for (int m = 0; m < p; ++m) {
    const int phase = (int)(((long)m * q + r.L) % p);
    for (int k = 0; k < r.K; ++k)
      if (phase + (long)p * k < ntaps) t[(size_t)k * p + m] = taps[phase + (long)p * k];
  }
  DS_HIP(hipGetDevice(&r.device));
  DS_HIP(hipMalloc(&r.tab, t.size() * sizeof(double)));
  if (hipMemcpy(r.tab, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(r.tab);
    DS_CHECK(false, "resampler_create: copying the tap table to the device failed");
  }
  *out = new diffsep_resampler(r);
  return 0;
}

extern "C" void diffsep_resampler_destroy(diffsep_resampler* r) {
  if (!r) return;
  (void)hipFree(r->tab);
  delete r;
}

extern "C" int32_t diffsep_resample(const diffsep_resampler* r, const float* x, int64_t ldx, void* y, int64_t ldy, int32_t rows,
                                    int64_t T, const int32_t* lengths, int32_t rows_per_length, int32_t* lengths_out,
                                    int32_t out_dtype, void* stream) {
  DS_CHECK(r && x && y, "resample: null pointer");
  DS_CHECK(out_dtype == DIFFSEP_F32 || out_dtype == DIFFSEP_F64, "resample: unknown out_dtype " + std::to_string(out_dtype) +
                                                                     " (DIFFSEP_F32 or DIFFSEP_F64)");
  DS_CHECK(rows >= 1 && rows <= 65535, "resample: rows must be in 1..65535 (" + std::to_string(rows) + ")");
  DS_CHECK(T >= 1 && T < ((int64_t)1 << 31), "resample: T must be in 1..2^31-1 (" + std::to_string(T) + ")");
  DS_CHECK(ldx >= T, "resample: ldx " + std::to_string(ldx) + " < T " + std::to_string(T));
  const int64_t nmax = (T * r->p + r->q - 1) / r->q;
  DS_CHECK(ldy >= nmax, "resample: ldy " + std::to_string(ldy) + " < ceil(T p / q) = " + std::to_string(nmax));
  DS_CHECK((nmax + kTile - 1) / kTile < ((int64_t)1 << 31), "resample: too many output tiles per row");
  DS_CHECK(!lengths_out || nmax < ((int64_t)1 << 31), "resample: lengths_out is int32 and ceil(T p / q) = " + std::to_string(nmax));
  DS_CHECK(rows_per_length >= 1, "resample: rows_per_length must be positive");
  int dev = 0;
  DS_HIP(hipGetDevice(&dev));
  DS_CHECK(dev == r->device, "resample: the resampler lives on device " + std::to_string(r->device) + ", the current device is " +
                                 std::to_string(dev));
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == DIFFSEP_F32) return rs_launch<float>(r, x, ldx, y, ldy, rows, T, nmax, lengths, rows_per_length, lengths_out, st);
  return rs_launch<double>(r, x, ldx, y, ldy, rows, T, nmax, lengths, rows_per_length, lengths_out, st);
}
