"""CPU ORACLE -- test infrastructure only, never the product path.

The reference's maketraj (control.py:63-197) as the least-squares problem it
poses (include/ikgrasp.h, ikg_bezier_fit_batch): its equality constraints pin
P[0..2] = q0 and P[d-2..d] = q1, and the d - 5 free control points minimise

    | A_f (X0_f + delta) + c - Y |^2 + ridge |delta|^2

with X0 = linspace(q0, q1, d + 1), A_f[k,i] = C(d,i) u_k^i (1 - u_k)^(d-i) for
i = 3 .. d-3 and c the pinned points' share.

  times     numpy's linspace(0, T, n) restated operation for operation, and u = t / T
  fit_f64   the float64 restatement: np.linalg.qr of the augmented [A_f; sqrt(ridge) 1]
  fit_mp    the same problem in 50-digit mpmath, solved exactly FROM THE FLOAT64 u_k
            (they are the inputs: both arithmetics see the same times)
  curve_mp / cost_mp   the Bernstein sum of a set of control points, in 50 digits
  horner    Bezier.eval_horner in float64 (the cost the kernel reports)

A 50-digit array travels as a double-double pair (hi, lo), hi + lo exact to
1e-32, so that an error of 1e-13 of max|P| is measured and not rounded away.
"""
from __future__ import annotations

from math import comb

import mpmath
import numpy as np

DPS = 50


def times(n, T):
    """-> (t [n], u [n]) float64: step = T / (n - 1), t_k = k step, t_{n-1} = T, u_k = t_k / T"""
    step = np.float64(T) / np.float64(n - 1)
    t = np.arange(n, dtype=np.float64) * step
    t[-1] = T
    assert np.array_equal(t, np.linspace(0, T, n))
    return t, t / np.float64(T)


def start_points(q0, q1, d):
    """X0 = linspace(q0, q1, d + 1) with the pinned points in place"""
    q0, q1 = np.asarray(q0, dtype=np.float64), np.asarray(q1, dtype=np.float64)
    X0 = q0 + np.arange(d + 1, dtype=np.float64)[:, None] * ((q1 - q0) / np.float64(d))
    X0[:3] = q0
    X0[d - 2:] = q1
    return X0


def bernstein(u, d):
    """[n, d + 1] float64"""
    u = np.asarray(u, dtype=np.float64)
    return np.array([[comb(d, i) * uk ** i * (1.0 - uk) ** (d - i) for i in range(d + 1)] for uk in u])


def fit_f64(q0, q1, y, T, d=20, ridge=0.0):
    """The float64 restatement -> P [d + 1, dim]"""
    y = np.asarray(y, dtype=np.float64)
    n, dim = y.shape
    m = d - 5
    _, u = times(n, T)
    A = bernstein(u, d)
    X0 = start_points(q0, q1, d)
    aug = np.vstack([A[:, 3:d - 2], np.sqrt(ridge) * np.eye(m)])
    rhs = np.vstack([y - A @ X0, np.zeros((m, dim))])
    Q, R = np.linalg.qr(aug)
    delta = np.linalg.solve(R, Q.T @ rhs)
    P = X0.copy()
    P[3:d - 2] += delta
    return P


def _mp_bernstein(u, d):
    rows = []
    for uk in u:
        x = mpmath.mpf(float(uk))
        rows.append([mpmath.binomial(d, i) * x ** i * (1 - x) ** (d - i) for i in range(d + 1)])
    return rows


def fit_mp(q0, q1, y, T, d=20, ridge=0.0):
    """The exact minimiser in 50 digits -> P as a [d + 1, dim] list of mpf rows.
    The normal equations are solved at 80 digits (cond^2 ~ 4e10 costs 11 of them)."""
    y = np.asarray(y, dtype=np.float64)
    n, dim = y.shape
    m = d - 5
    _, u = times(n, T)
    with mpmath.workdps(80):
        A = _mp_bernstein(u, d)
        X0 = [[mpmath.mpf(float(x)) for x in row] for row in start_points(q0, q1, d)]
        Af = mpmath.matrix([[A[k][3 + c] for c in range(m)] for k in range(n)])
        rhs = mpmath.matrix(n, dim)
        for k in range(n):
            for j in range(dim):
                rhs[k, j] = mpmath.mpf(float(y[k, j])) - mpmath.fsum(A[k][i] * X0[i][j] for i in range(d + 1))
        N = Af.T * Af + mpmath.mpf(float(ridge)) * mpmath.eye(m)
        g = Af.T * rhs
        P = [list(row) for row in X0]
        for j in range(dim):
            delta = mpmath.lu_solve(N, g[:, j])
            for c in range(m):
                P[3 + c][j] = X0[3 + c][j] + delta[c]
    return P


def curve_mp(P, u, d):
    """Bernstein sum at the float64 parameters u -> [len(u), dim] list of mpf rows"""
    with mpmath.workdps(DPS):
        A = _mp_bernstein(u, d)
        dim = len(P[0])
        return [[mpmath.fsum(A[k][i] * P[i][j] for i in range(d + 1)) for j in range(dim)] for k in range(len(u))]


def cost_mp(P, y, T, d):
    y = np.asarray(y, dtype=np.float64)
    _, u = times(len(y), T)
    with mpmath.workdps(DPS):
        c = curve_mp(P, u, d)
        return mpmath.fsum((c[k][j] - mpmath.mpf(float(y[k, j]))) ** 2 for k in range(len(y)) for j in range(y.shape[1]))


def to_mp(P):
    return [[mpmath.mpf(float(x)) for x in row] for row in np.asarray(P, dtype=np.float64)]


def split(X):
    """list of mpf rows -> (hi, lo) float64 arrays with hi + lo = X to 1e-32"""
    hi = np.array([[float(x) for x in row] for row in X])
    lo = np.array([[float(x - mpmath.mpf(h)) for x, h in zip(row, hrow)] for row, hrow in zip(X, hi)])
    return hi, lo


def diff(P, hi, lo):
    """P - (hi + lo) in float64 without losing the difference"""
    return (np.asarray(P, dtype=np.float64) - hi) - lo


def horner(P, t, T):
    """Bezier(P, 0, T)(t), eval_horner operation for operation (control.py:38-46), float64"""
    P = np.asarray(P, dtype=np.float64)
    d = len(P) - 1
    u = (np.float64(t) - 0.0) / (np.float64(T) - 0.0)
    uo, bc, tn = 1.0 - u, 1.0, 1.0
    tmp = P[0] * uo
    for i in range(1, d):
        tn *= u
        bc *= (d - i + 1) / i
        tmp = (tmp + tn * bc * P[i]) * uo
    return tmp + tn * u * P[-1]


def cost_f64(P, y, T):
    """The reference's cost_function (control.py:96-104) in float64"""
    y = np.asarray(y, dtype=np.float64)
    t, _ = times(len(y), T)
    cost = 0.0
    for tk, yk in zip(t, y):
        cost += np.sum((horner(P, tk, T) - yk) ** 2)
    return cost


CURVE_U = np.arange(64, dtype=np.float64) / 63.0  # the 64 evenly spaced parameters of the curve check
