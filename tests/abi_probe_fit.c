/* Sizes and field offsets of the fit and per-state rollout structures of
 * include/ikgrasp.h, one "struct field offset size" line each
 * (tests/test_fit.py compares them with ikgrasp/_lib.py). */
#include <stddef.h>
#include <stdio.h>

#include "ikgrasp.h"

#define F(S, f) printf(#S " " #f " %zu %zu\n", offsetof(S, f), sizeof(((S*)0)->f))
#define SZ(S) printf(#S " sizeof 0 %zu\n", sizeof(S))

int main(void) {
  F(ikg_bezier_set, points);
  F(ikg_bezier_set, n_points);
  F(ikg_bezier_set, t_min);
  F(ikg_bezier_set, t_max);
  F(ikg_bezier_set, mult);
  SZ(ikg_bezier_set);
  F(ikg_fit_params, degree);
  F(ikg_fit_params, ridge);
  F(ikg_fit_params, total_time);
  SZ(ikg_fit_params);
  return 0;
}
