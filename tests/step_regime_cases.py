"""What tests/golden/make_step_regime_golden.py, tests/test_step_regime.py and
tests/test_gpu_step_regime.py share: the step-size regimes of the IK loop's
carried joint trig (ikg_device.hpp Trig<T>), the case list of
tests/golden/step_regime_cases.npz and its loader.  numpy only.

The loop carries sin q / cos q and advances them by the joint step d:
  short   |d| <= kIncMax (fp64 0.025, fp32 0.1)   three in-place shears
  medium  |d| <= kIncMed (fp64 0.25,  fp32 0.5)   the longer series
  exact   beyond, and at resyncs                 sincos of the angle
The generic kernels threshold the seven joint steps of an arm lane (chest +
six arm joints), the frame-1 kernels its seven slot steps, two of which are
sums of two joint steps (SLOT_SUMS)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(GOLDEN, "step_regime_cases.npz")
TILTED_PATH = os.path.join(GOLDEN, "step_regime_tilted.npz")

THR = {"f64": (0.025, 0.25), "f32": (0.1, 0.5)}  # Trig<T>::kIncMax, kIncMed
PRECS = ("f64", "f32")
K_INC_ASIN = 0.035  # ThetaInc<T>::kIncAsin: the angle tracker is incremental while |sin(dtheta)| <= this
EDGE = 0.01         # a step within 1 % of a threshold counts for no coverage condition
SHORT, MEDIUM, EXACT, AT_EDGE, UNUSED = 0, 1, 2, -1, -2

LAYOUTS = ("zero", "rows")  # q0 = 0 broadcast / one seed row per problem
DTS = (1e-2, 0.05, 0.25, 1.0)
KS = (1, 2, 4, 8)
K_TOP = 8
N_A = 32
C_DTS = (0.05, 0.1, 0.25)
D_DTS = (0.05, 0.25)
N_D = 64
LAMBDA = 1e-6  # the damped route's lambda
B_K = 2  # group B: the first update lands on the threshold, the second consumes the advanced trig

# the tilted robot (tests/golden/tilted_dualarm.urdf, generic and run-time-compiled kernels): rows of
# generic_cases.npz, 8 from q0 = 0 and 8 from the perturbed posture, each with its own q0 row
T_ROWS = tuple(range(8)) + tuple(range(24, 32))
T_KS = (1, 2, 4)


def t_cases():
    """[(dt, K)] of the tilted robot's fixture, in its order."""
    return [(dt, k) for dt in DTS for k in T_KS if k <= max(ks_for(dt))]


ROOT_Q = 0
ARM_Q = ((3, 4, 5, 6, 7, 8), (9, 10, 11, 12, 13, 14))
SLOT_SUMS = {0: (0, 1), 3: (2, 3)}  # slot -> the two lane joints whose steps it adds (trig_advance_f1)


def ks_for(dt):
    """The loop is chaotic at dt = 1: its C and numpy float64 restatements part by 6.6e-8 at K = 4."""
    return tuple(k for k in KS if k <= 2) if dt >= 1.0 else KS


def a_cases():
    """[(layout, dt, K)] in the fixture's order."""
    return [(lay, dt, k) for lay in LAYOUTS for dt in DTS for k in ks_for(dt)]


def a_index(layout, dt, K):
    return a_cases().index((layout, dt, K))


def lane_steps(q_old, q_new):
    """[..., 15] iterates -> (joint steps, slot steps), each [..., 2 arms, 7]."""
    d = np.asarray(q_new, dtype=np.float64) - np.asarray(q_old, dtype=np.float64)
    dj = np.stack([np.concatenate([d[..., [ROOT_Q]], d[..., list(a)]], axis=-1) for a in ARM_Q], axis=-2)
    ds = dj.copy()
    for s, (i, j) in SLOT_SUMS.items():
        ds[..., s] = dj[..., i] + dj[..., j]
    return dj, ds


def regime(x, prec):
    """Largest |step| -> SHORT / MEDIUM / EXACT, AT_EDGE within 1 % of a threshold."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    lo, hi = THR[prec]
    r = np.where(x > hi, EXACT, np.where(x > lo, MEDIUM, SHORT)).astype(np.int8)
    for t in (lo, hi):
        r = np.where(np.abs(x - t) <= EDGE * t, AT_EDGE, r).astype(np.int8)
    return r


def load():
    """The fixture, with the C oracle's q rebuilt from the 32-digit q and the
    stored difference of their bit patterns."""
    d = dict(np.load(PATH))
    for g in ("a", "b"):
        d[f"{g}_q_c"] = (np.ascontiguousarray(d[f"{g}_q_mp"]).view(np.int64) + d[f"{g}_dq_c"]).view(np.float64)
    return d


def load_tilted():
    d = dict(np.load(TILTED_PATH))
    d["t_q_ref"] = (np.ascontiguousarray(d["t_q_mp"]).view(np.int64) + d["t_dq_ref"]).view(np.float64)
    return d


def a_regimes(d, layout, dt, K, kind, prec):
    """Regime codes [K, 32, 2 arms] of the updates 1..K of a group-A case;
    kind 'joint' (generic kernels) or 'slot' (frame-1 kernels)."""
    r = d["a_regime"][LAYOUTS.index(layout), DTS.index(dt), :K, :, :, ("joint", "slot").index(kind), PRECS.index(prec)]
    assert (r != UNUSED).all()
    return r
