/* Prints "<struct> <field> <offset> <size>" for every field of the controller
 * dynamics structures of include/ikgrasp.h, and "<struct> sizeof 0 <size>";
 * tests/test_dynamics.py compares them with the ctypes mirrors in ikgrasp/_lib.py. */
#include <stddef.h>
#include <stdio.h>

#include "ikgrasp.h"

#define F(S, f) printf(#S " " #f " %zu %zu\n", offsetof(S, f), sizeof(((S*)0)->f))
#define Z(S) printf(#S " sizeof 0 %zu\n", sizeof(S))

int main(void) {
  F(ikg_inertia_desc, mass);
  F(ikg_inertia_desc, com);
  F(ikg_inertia_desc, inertia);
  F(ikg_inertia_desc, gravity);
  Z(ikg_inertia_desc);
  F(ikg_dynamics_out, M);
  F(ikg_dynamics_out, nle);
  F(ikg_dynamics_out, g);
  Z(ikg_dynamics_out);
  F(ikg_control_params, Kp);
  F(ikg_control_params, Kv);
  F(ikg_control_params, Kf);
  F(ikg_control_params, Kt);
  F(ikg_control_params, lambda_reg);
  F(ikg_control_params, qp_reg);
  F(ikg_control_params, fc_bias);
  F(ikg_control_params, zero_tau_mask);
  Z(ikg_control_params);
  F(ikg_control_out, tau);
  F(ikg_control_out, qdd);
  F(ikg_control_out, xdd);
  F(ikg_control_out, Lambda);
  F(ikg_control_out, fc);
  Z(ikg_control_out);
  return 0;
}
