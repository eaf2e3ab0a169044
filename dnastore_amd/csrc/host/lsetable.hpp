// The reference's log-sum-exp by table (logsumexp.h:19-74, logsumexp.cpp:5-19), stated once for the host: the 100 001-entry
// table of log(1 + exp(-x)) at x = n * 1e-4 that every runtime uploads, and the function over it that the device code
// (fwdback_kernels.hip, fwdback_onchip.hip, pair_forward_device.h) restates operation for operation.  Only the host libm ever
// evaluates log and exp; the device loads, adds and multiplies.
#pragma once
#include <cmath>
#include <limits>
#include <mutex>
#include <vector>

namespace dnas {

constexpr int kLseTableSize = 100001;      // ((int)(10 / .0001)) + 1

inline const std::vector<double>& lseTable() {
  static std::vector<double> tab;
  static std::once_flag once;
  std::call_once(once, [] {
    const int n = ((int)(10 / .0001)) + 1;
    tab.resize(n);
    for (int i = 0; i < n; ++i) tab[i] = std::log(1. + std::exp(-(i * .0001)));
  });
  return tab;
}

// log(1 + exp(-x)) for x >= 0: 0 from 10 on (and for the NaN / +inf a difference of infinities gives), else the table
// interpolated linearly.  x < 10 gives n <= 99 999, so tab[n + 1] exists.
inline double lseUnaryTable(const double* tab, double x) {
  if (x >= 10. || x != x || x == std::numeric_limits<double>::infinity()) return 0;
  if (x < 0) return -x;
  const int n = (int)(x / .0001);
  const double dx = x - (n * .0001);
  const double f0 = tab[n], f1 = tab[n + 1];
  const double df = f1 - f0;
  return f0 + df * (dx / .0001);
}

// log(exp(a) + exp(b)): lse(-inf, -inf) = -inf, lse(x, -inf) = x exactly.
inline double lseTableSum(const double* tab, double a, double b) {
  double mx, diff;
  if (a == b) { mx = a; diff = 0; }
  else if (a < b) { mx = b; diff = b - a; }
  else { mx = a; diff = a - b; }
  return mx + lseUnaryTable(tab, diff);
}

// The same sum with the host libm in place of the table (host only).
inline double lseExactSum(double a, double b) {
  double mx, diff;
  if (a == b) { mx = a; diff = 0; }
  else if (a < b) { mx = b; diff = b - a; }
  else { mx = a; diff = a - b; }
  if (diff != diff || diff == std::numeric_limits<double>::infinity()) return mx;
  return mx + std::log1p(std::exp(-diff));
}

}  // namespace dnas
