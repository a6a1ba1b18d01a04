// The built-in Slaney mel basis and the window | cos | sin table of the 1024-point transform, shared by the filterbank (fbank.hip)
// and its inverse (vocoder.hip).  Host code only.
#pragma once
#include <math.h>

#include <algorithm>
#include <vector>

namespace vx __attribute__((visibility("hidden"))) {

// Slaney's mel scale (Auditory Toolbox): linear below 1 kHz at 200 / 3 Hz per mel, logarithmic above with step log(6.4) / 27.
inline double hz_to_mel(double f) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, logstep = log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_hz / f_sp + log(f / min_log_hz) / logstep : f / f_sp;
}
inline double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// Triangular filters between n_mels + 2 points equally spaced in mel, each scaled by 2 / (its width in Hz): (n_mels x n_bins) fp64.
inline std::vector<double> slaney_basis_f64(int sr, int n_mels, int n_bins, double fmin, double fmax) {
  std::vector<double> pts(n_mels + 2);
  const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax);
  for (int i = 0; i < n_mels + 2; ++i) pts[i] = mel_to_hz(m0 + (m1 - m0) * (double)i / (double)(n_mels + 1));
  std::vector<double> w((size_t)n_mels * n_bins);
  for (int i = 0; i < n_mels; ++i) {
    const double norm = 2.0 / (pts[i + 2] - pts[i]);
    for (int b = 0; b < n_bins; ++b) {
      const double f = 0.5 * (double)sr * (double)b / (double)(n_bins - 1);
      const double lower = (f - pts[i]) / (pts[i + 1] - pts[i]), upper = (pts[i + 2] - f) / (pts[i + 2] - pts[i + 1]);
      w[(size_t)i * n_bins + b] = std::max(0.0, std::min(lower, upper)) * norm;
    }
  }
  return w;
}

// The same table rounded once to fp32.
inline std::vector<float> slaney_basis(int sr, int n_mels, int n_bins, double fmin, double fmax) {
  const std::vector<double> w = slaney_basis_f64(sr, n_mels, n_bins, fmin, fmax);
  return std::vector<float>(w.begin(), w.end());
}

// The tables of the 1024-point transform both units run: periodic Hann [1024] | cos [1024] | sin [1024] of 2 pi j / 1024, in
// fp64, rounded once.  The vocoder appends columns of its own.
inline std::vector<float> hann_cos_sin_1024() {
  std::vector<float> tab(3 * 1024);
  const double pi = 3.14159265358979323846;
  for (int j = 0; j < 1024; ++j) {
    const double t = 2.0 * pi * (double)j / 1024.0;
    tab[j] = (float)(0.5 - 0.5 * cos(t));
    tab[1024 + j] = (float)cos(t);
    tab[2048 + j] = (float)sin(t);
  }
  // the multiples of a quarter turn exactly (cos(pi / 2) in fp64 is 6e-17, not 0)
  tab[1024 + 256] = 0.f; tab[1024 + 768] = 0.f; tab[2048 + 512] = 0.f;
  return tab;
}

}  // namespace vx
