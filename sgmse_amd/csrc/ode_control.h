// Host side of the adaptive probability-flow sampler: scipy's RK45 step control (scipy/integrate/_ivp/rk.py RungeKutta._step_impl,
// common.py select_initial_step) for ONE integration, in double.  Engine::ode_run drives one controller per group: one for the whole
// flattened batch, or one per utterance; nothing but the code below decides a step, so an utterance integrated alone and the same
// utterance inside a batch take the same steps from the same norms.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace sgmse {

struct OdeControl {
  // Dormand-Prince 5(4) tableau (rk.py RK45)
  static constexpr double C[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};
  static constexpr double A[6][5] = {{0, 0, 0, 0, 0},
                                     {1.0 / 5, 0, 0, 0, 0},
                                     {3.0 / 40, 9.0 / 40, 0, 0, 0},
                                     {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
                                     {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
                                     {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
  static constexpr double Bw[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
  static constexpr double E[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};

  double t = 0.0, t_stop = 0.0, dir = -1.0, interval = 0.0, max_step = INFINITY;
  double n = 1.0;                 // complex elements the norms run over
  double h_abs = 0.0;             // size of the next attempt
  double h0 = 0.0, d1 = 0.0;      // select_initial_step, between its two norm passes
  double min_step = 0.0, h = 0.0, t_new = 0.0;      // the attempt in flight
  bool fresh = true;              // the next attempt is the first of a step
  bool rejected = false;          // the step in progress has had an attempt rejected
  int nfe = 0, n_accepted = 0, n_rejected = 0;
  std::vector<double> t_accepted;

  void start(double t0, double t_end, double max_step_or_0, double n_elements) {
    *this = OdeControl();
    t = t0; t_stop = t_end; n = n_elements;
    interval = std::fabs(t_end - t0); dir = t_end < t0 ? -1.0 : 1.0;
    max_step = max_step_or_0 > 0 ? max_step_or_0 : INFINITY;
  }
  bool done() const { return !(dir * (t - t_stop) < 0); }
  double last_time(double t0) const { return t_accepted.empty() ? t0 : t_accepted.back(); }

  // select_initial_step (Hairer, Norsett, Wanner I, II.4), error estimator order 4.  s0, s1: the sums of ode_init_norms_each_kernel.
  // First pass (x, K_0) -> the probe step h0: the probe evaluation is at t + h0 dir, its stage coefficient h0 dir.
  double probe_step(double s0, double s1) {
    const double d0 = std::sqrt(s0 / n);
    d1 = std::sqrt(s1 / n);
    h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    h0 = std::min(h0, interval);
    return h0;
  }
  // Second pass (K at the probe - K_0) -> the first step
  void first_step_from_probe(double s1) {
    const double d2 = std::sqrt(s1 / n) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0 * 1e-3) : std::pow(0.01 / std::max(d1, d2), 1.0 / 5.0);
    h_abs = std::min(std::min(100.0 * h0, h1), std::min(interval, max_step));
  }

  // The next attempt's h and t_new.  False: the step size fell below 10 ulp(t) ("required step size is less than spacing between
  // numbers").
  bool begin_attempt() {
    if (fresh) {
      min_step = 10.0 * std::fabs(std::nextafter(t, dir * INFINITY) - t);
      if (h_abs > max_step) h_abs = max_step;
      else if (h_abs < min_step) h_abs = min_step;
      rejected = false;
      fresh = false;
    }
    if (h_abs < min_step) return false;
    h = h_abs * dir; t_new = t + h;
    if (dir * (t_new - t_stop) > 0) t_new = t_stop;
    h = t_new - t;
    h_abs = std::fabs(h);
    return true;
  }
  // The attempt's six stage times and the coefficient columns [1..] of its table rows 0..6 (kernels_ode.h; `table` zeroed by the
  // caller, rows `stride` doubles apart; column 0, g(t)^2 / 2, is the caller's).
  void fill_attempt(double* times, double* table, int stride) const {
    for (int e = 0; e < 5; ++e) times[e] = t + C[e + 1] * h;
    times[5] = t + h;
    for (int e = 0; e < 4; ++e) for (int j = 0; j <= e + 1; ++j) table[e * stride + 1 + j] = h * A[e + 2][j];
    for (int j = 0; j < 6; ++j) table[4 * stride + 1 + j] = h * Bw[j];
    for (int j = 0; j < 7; ++j) table[5 * stride + 1 + j] = h * E[j];
    table[6 * stride + 1] = h * A[1][0];
  }
  // s0: the sum of ode_error_each_kernel.  True: accepted (t advanced, "first same as last": the caller makes x <- y_new, K_0 <- K_6).
  bool finish_attempt(double s0) {
    const double norm = std::sqrt(s0 / n);
    if (norm < 1.0) {
      double factor = norm == 0.0 ? 10.0 : std::min(10.0, 0.9 * std::pow(norm, -0.2));
      if (rejected) factor = std::min(1.0, factor);
      h_abs *= factor;
      t = t_new;
      ++n_accepted;
      t_accepted.push_back(t);
      fresh = true;
      return true;
    }
    const double shrink = 0.9 * std::pow(norm, -0.2);
    h_abs *= shrink > 0.2 ? shrink : 0.2;      // (a non-finite norm is a rejection with the smallest factor, as max(MIN_FACTOR, nan) is in scipy)
    rejected = true;
    ++n_rejected;
    return false;
  }
};

}  // namespace sgmse
