/* Prints "<struct> <field> <offset> <size>" for every field of the rollout
 * structures of include/ikgrasp.h, and "<struct> sizeof 0 <size>";
 * tests/test_rollout.py compares them with the ctypes mirrors in ikgrasp/_lib.py. */
#include <stddef.h>
#include <stdio.h>

#include "ikgrasp.h"

#define F(S, f) printf(#S " " #f " %zu %zu\n", offsetof(S, f), sizeof(((S*)0)->f))
#define Z(S) printf(#S " sizeof 0 %zu\n", sizeof(S))

int main(void) {
  F(ikg_bezier, points);
  F(ikg_bezier, n_points);
  F(ikg_bezier, t_min);
  F(ikg_bezier, t_max);
  F(ikg_bezier, mult);
  Z(ikg_bezier);
  F(ikg_rollout_params, control);
  F(ikg_rollout_params, dt_sim);
  F(ikg_rollout_params, dt_traj);
  F(ikg_rollout_params, ticks);
  F(ikg_rollout_params, record_every);
  Z(ikg_rollout_params);
  F(ikg_rollout_out, q);
  F(ikg_rollout_out, v);
  F(ikg_rollout_out, t);
  F(ikg_rollout_out, q_hist);
  F(ikg_rollout_out, v_hist);
  F(ikg_rollout_out, tau_hist);
  Z(ikg_rollout_out);
  return 0;
}
