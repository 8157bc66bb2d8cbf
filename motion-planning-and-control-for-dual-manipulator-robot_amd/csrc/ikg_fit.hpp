// Bezier trajectory fit (control.py:63-197, maketraj) as the linear
// least-squares problem it poses.  The reference's six equality constraints pin
// P[0..2] = q0 and P[d-2..d] = q1; the d - 5 free control points minimise
//   | A_f (X0_f + delta) + c - Y |^2 + ridge |delta|^2
// with A_f[k,i] = C(d,i) u_k^i (1 - u_k)^(d-i), i = 3 .. d-3, c the pinned
// points' share and X0 = linspace(q0, q1, d + 1), the reference's initial guess.
// cond(A_f) is about 2e5 at degree 20, so the normal equations lose the control
// points (1e-3 .. 4e-2); the solve is a Householder factorisation of the
// augmented matrix [A_f | Y - A X0; sqrt(ridge) 1 | 0], every right-hand side
// (one per joint) carried along, then a back substitution per joint.
//
// The phases are written once over an executor `ex`: ex(count, fn) runs fn(i)
// for i in [0, count) and then makes the writes visible to every item.  The
// kernel's executor strides the items over the workgroup's lanes and ends with
// a barrier (ikg_fit.hip); the host's is a loop (ikg_host_emu.hip).  No phase
// reads what another item of the same phase writes.
#pragma once

#include "ikg_dynamics.hpp"

namespace ikg {

constexpr int kFitMaxN = 256;      // path points
constexpr int kFitMinDegree = 6;   // one free control point
constexpr int kFitMaxDegree = 20;  // the reference's
constexpr int kFitMaxFree = kFitMaxDegree - 5;
constexpr int kFitParts = 8;    // row slices of a column's dot product
constexpr int kFitLanes = 256;  // partial sums of the cost (and the kernel's workgroup)

// one path of the batch
struct FitPath {
  const double *q0, *q1;  // [dim]
  const double* y;        // [n, dim]
  int n, dim, degree;
  double ridge, T;
  const double* bc;  // [degree + 1] bezier_coeffs
};

// workspace of one path, in doubles (LDS in the kernel)
struct FitWs {
  double* W;     // [(kFitMaxN + m), m + dim] row-major: [A_f | rhs], then the ridge rows
  double* P;     // [degree + 1, dim]
  double* part;  // [kFitParts, m + dim]
  double* dot;   // [m + dim]
  double* diag;  // [m]
  double* red;   // [kFitLanes + 16]
};

IKG_HD inline size_t fit_ws_len(int degree, int dim) {
  const int m = degree - 5, nc = m + dim;
  return (size_t)(kFitMaxN + m) * nc + (size_t)(degree + 1) * dim + (size_t)kFitParts * nc + nc + m + kFitLanes + 16;
}

IKG_HD inline void fit_ws_bind(double* base, int degree, int dim, FitWs& w) {
  const int m = degree - 5, nc = m + dim;
  w.W = base;
  w.P = w.W + (size_t)(kFitMaxN + m) * nc;
  w.part = w.P + (size_t)(degree + 1) * dim;
  w.dot = w.part + (size_t)kFitParts * nc;
  w.diag = w.dot + nc;
  w.red = w.diag + m;
}

// the path's count is usable: the kernel checks it before anything is indexed by it
IKG_HD inline bool fit_count_ok(int64_t n, int degree, double ridge) {
  return n >= 2 && n <= kFitMaxN && (ridge > 0.0 || n >= degree - 3);
}

// numpy's linspace(0, T, n)[k]: k * (T / (n - 1)), the last one T itself
IKG_HD inline double fit_time(int k, int n, double T) {
  return k == n - 1 ? T : (double)k * (T / (double)(n - 1));
}

// row k < n of [A_f | y - B(u_k; X0 with the pinned points)]; w.P holds that X0
IKG_HD inline void fit_row(const FitPath& f, const FitWs& w, int k) {
  const int d = f.degree, m = d - 5, ld = m + f.dim;
  const double u = fit_time(k, f.n, f.T) / f.T, uo = 1.0 - u;
  double b[kFitMaxDegree + 1];
  double pw = 1.0;
#pragma unroll
  for (int i = 0; i <= kFitMaxDegree; ++i)
    if (i <= d) {
      b[i] = f.bc[i] * pw;
      pw *= u;
    }
  pw = 1.0;
#pragma unroll
  for (int i = kFitMaxDegree; i >= 0; --i)
    if (i <= d) {
      b[i] *= pw;
      pw *= uo;
    }
  double* row = w.W + (size_t)k * ld;
#pragma unroll
  for (int c = 0; c < kFitMaxFree; ++c)
    if (c < m) row[c] = b[3 + c];
  for (int j = 0; j < f.dim; ++j) {
    double acc = f.y[(size_t)k * f.dim + j];
#pragma unroll
    for (int i = 0; i <= kFitMaxDegree; ++i)
      if (i <= d) acc -= b[i] * w.P[i * f.dim + j];
    row[m + j] = acc;
  }
}

// derivative control points exactly as Bezier.derivative forms them: degree (P[i+1] - P[i])
IKG_HD inline double fit_vpoint(const double* P, int dim, int degree, int e) {
#pragma clang fp contract(off)
  return (double)degree * (P[e + dim] - P[e]);
}
IKG_HD inline double fit_apoint(const double* P, int dim, int degree, int e) {
#pragma clang fp contract(off)
  return (double)(degree - 1) * (fit_vpoint(P, dim, degree, e + dim) - fit_vpoint(P, dim, degree, e));
}

// The fit of one path whose count passed fit_count_ok.  points [degree + 1, dim];
// vpoints [degree, dim] and apoints [degree - 1, dim] may be null.  Returns the
// cost sum_k sum_j (B(t_k)_j - y_kj)^2 with the reference's Horner (bezier_eval).
template <typename Ex>
IKG_HD inline double bezier_fit_path(const FitPath& f, const FitWs& w, Ex& ex, double* points, double* vpoints,
                                     double* apoints) {
  const int d = f.degree, dim = f.dim, n = f.n;
  const int m = d - 5, nc = m + dim, ld = nc, M = n + m;
  double* W = w.W;
  // X0 = linspace(q0, q1, d + 1) with the pinned points in place; numpy's
  // rounding (a product, then a sum), so that a path that moves nothing
  // (n = 2: A_f = 0) returns the reference's initial guess bit for bit
  ex((d + 1) * dim, [&](int e) {
#pragma clang fp contract(off)
    const int i = e / dim, j = e % dim;
    const double a = f.q0[j], b = f.q1[j];
    w.P[e] = i <= 2 ? a : (i >= d - 2 ? b : a + (double)i * ((b - a) / (double)d));
  });
  const double sr = sqrt(f.ridge);
  ex(M, [&](int r) {
    if (r < n) {
      fit_row(f, w, r);
    } else {
      for (int c = 0; c < nc; ++c) W[(size_t)r * ld + c] = c == r - n ? sr : 0.0;
    }
  });
  // Householder, a reflection per free column: v = x - alpha e_k, alpha = -sign(x_k) |x|
#pragma unroll 1
  for (int k = 0; k < m; ++k) {
    const int ncol = nc - k;
    ex(ncol * kFitParts, [&](int i) {
      const int c = k + i / kFitParts, part = i % kFitParts;
      double acc = 0.0;
      for (int r = k + part; r < M; r += kFitParts) acc += W[(size_t)r * ld + k] * W[(size_t)r * ld + c];
      w.part[i] = acc;
    });
    ex(ncol, [&](int i) {
      double sigma = 0.0, di = 0.0;
      for (int s = 0; s < kFitParts; ++s) {
        sigma += w.part[s];
        di += w.part[i * kFitParts + s];
      }
      const double xk = W[(size_t)k * ld + k];
      const double nrm = sqrt(sigma);
      const double alpha = xk > 0.0 ? -nrm : nrm;
      // (v . W_c) 2 / (v . v), v . v = 2 (sigma - x_k alpha)
      w.dot[i] = sigma > 0.0 ? (di - alpha * W[(size_t)k * ld + k + i]) / (sigma - xk * alpha) : 0.0;
      if (i == 0) w.diag[k] = alpha;
    });
    ex((M - k) * (ncol - 1), [&](int e) {
      const int r = k + e / (ncol - 1), c = k + 1 + e % (ncol - 1);
      const double vr = r == k ? W[(size_t)k * ld + k] - w.diag[k] : W[(size_t)r * ld + k];
      W[(size_t)r * ld + c] -= w.dot[c - k] * vr;
    });
  }
  // R delta = Q^T rhs, a joint per item; delta replaces the right-hand side
  ex(dim, [&](int j) {
    for (int i = m - 1; i >= 0; --i) {
      double acc = W[(size_t)i * ld + m + j];
      for (int c = i + 1; c < m; ++c) acc -= W[(size_t)i * ld + c] * W[(size_t)c * ld + m + j];
      W[(size_t)i * ld + m + j] = acc / w.diag[i];
    }
  });
  ex(m * dim, [&](int e) { w.P[3 * dim + e] += W[(size_t)(e / dim) * ld + m + e % dim]; });
  ex((d + 1) * dim, [&](int e) {
    points[e] = w.P[e];
    if (vpoints && e < d * dim) vpoints[e] = fit_vpoint(w.P, dim, d, e);
    if (apoints && e < (d - 1) * dim) apoints[e] = fit_apoint(w.P, dim, d, e);
  });
  const KBezier<double> kb{w.P, f.bc, d + 1, dim, 0.0, f.T, 1.0};
  ex(kFitLanes, [&](int t) {
    double acc = 0.0;
    for (int e = t; e < n * dim; e += kFitLanes) {
      const double r = bezier_eval(kb, fit_time(e / dim, n, f.T), e % dim) - f.y[e];
      acc += r * r;
    }
    w.red[t] = acc;
  });
  ex(16, [&](int t) {
    double acc = 0.0;
    for (int i = 0; i < kFitLanes / 16; ++i) acc += w.red[t * (kFitLanes / 16) + i];
    w.red[kFitLanes + t] = acc;
  });
  double cost = 0.0;
  for (int t = 0; t < 16; ++t) cost += w.red[kFitLanes + t];
  return cost;
}

// quiet NaN by its bits (the device code is built with -ffinite-math-only)
IKG_HD inline void fit_store_nan(double* x) { *reinterpret_cast<unsigned long long*>(x) = 0x7ff8000000000000ull; }

}  // namespace ikg
