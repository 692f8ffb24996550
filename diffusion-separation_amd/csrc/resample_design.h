// resample_design.h — the project's one anti-aliasing filter design (host only): Octave's resample(x, p, q), a Kaiser-windowed sinc
// with 60 dB rejection, as diffsep_amd/metrics.py (_resample_filter) states it.  stoi.hip (to 10 kHz) and resample.hip (any
// reduced p / q) both build their taps here: the same operations, the same roundings.
#pragma once

#include <cmath>

namespace {

constexpr int kResampleMaxRatio = 1000;  // largest p or q a tap table is designed for

// half-length L of the filter of the reduced ratio p / q (2 L + 1 taps); p = q = 1: 0 (one tap, a copy)
inline int ds_resample_half_length(int p, int q) {
  if (p == 1 && q == 1) return 0;
  const int m = p > q ? p : q;
  const double fc = 1.0 / (2.0 * m);
  return (int)std::ceil((60.0 - 8.0) / (28.714 * fc / 10.0));
}

// taps[0 .. 2 L] of the reduced ratio p / q, scaled so that they sum to p (unit DC gain after the zero stuffing)
inline void ds_resample_design(int p, int q, int L, double* taps) {
  const double pi = 3.14159265358979323846;
  if (L <= 0) {
    taps[0] = 1.0;
    return;
  }
  const int m = p > q ? p : q;
  const double fc = 1.0 / (2.0 * m), beta = 0.1102 * (60.0 - 8.7), i0b = std::cyl_bessel_i(0.0, beta);
  double sum = 0.0;
  for (int k = 0; k <= 2 * L; ++k) {
    const double tt = (double)(k - L), u = tt / L, a = 2.0 * fc * tt;
    const double win = std::cyl_bessel_i(0.0, beta * std::sqrt(std::fmax(0.0, 1.0 - u * u))) / i0b;
    const double sinc = (k == L) ? 1.0 : std::sin(pi * a) / (pi * a);
    taps[k] = win * (2.0 * p * fc * sinc);
    sum += taps[k];
  }
  for (int k = 0; k <= 2 * L; ++k) taps[k] = taps[k] / sum * p;
}

}  // namespace
