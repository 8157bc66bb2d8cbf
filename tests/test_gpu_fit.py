"""The Bezier trajectory fit and the per-state rollout on the GPU
(ikg_bezier_fit_batch, ikg_control_rollout_curves) against
tests/golden/fit_cases.npz (make_fit_golden.py): the control points, the curve
and the cost under tol_P / tol_curve / tol_cost as stored in the fixture (20 x
the float64 restatement's error against the 50-digit minimiser), the
reference's own maketraj results, and bit-equality between calls."""
import numpy as np
import pytest

import fit_cases as fc
import rollout_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def d():
    return fc.load()


@pytest.fixture(scope="module")
def rd():
    return rc.load()


def _dev(x, dtype=None):
    import torch
    return torch.tensor(np.asarray(x), device="cuda", dtype=dtype or torch.float64)


def _dev_fit(solver):
    """bezier_fit with every array a device tensor (offsets included)"""
    import torch

    def fit(q0, q1, y, off, **kw):
        r = solver.bezier_fit(_dev(q0), _dev(q1), _dev(y), _dev(off, torch.int64), **kw)
        torch.cuda.synchronize()
        return r
    return fit


# ---------------------------------------------------------------- against the fixture
@pytest.mark.parametrize("name", list(fc.CASES))
def test_fit_within_measured_bounds(solver, d, name):
    r = fc.check_case(solver.bezier_fit, d, name, "gpu")
    fc.check_derivatives(r, fc.CASES[name][2])


@pytest.mark.parametrize("name", fc.REFERENCE)
def test_not_above_the_references_cost(solver, d, name):
    fc.check_reference(solver.bezier_fit, d, name)


def test_ragged_batch_equals_one_path_per_call(solver, d):
    fc.check_ragged(solver.bezier_fit, d)


def test_device_pointers_equal_host_pointers(solver, d):
    host = fc.check_ragged(solver.bezier_fit, d)
    dev = fc.check_ragged(_dev_fit(solver), d)
    for k in ("points", "vpoints", "apoints", "cost", "status"):
        assert np.array_equal(host[k], dev[k]), k
    fc.check_case(_dev_fit(solver), d, "n40w", "gpu, device pointers")


def test_count_out_of_range_is_refused_in_the_kernel(solver, d):
    """Device pointers: the host cannot see the counts, so the kernel checks each
    before it sizes or indexes anything: status 1, cost NaN, points untouched,
    neighbours as solved alone.  Every offset lies inside the buffer."""
    import torch
    q0, q1, y = fc.inputs(d, "n40")
    long = np.vstack([d["n256_y"], d["n256_y"][:44]])  # 300 points: above the cap
    yy, off = fc.pack([y, long, y, y[:16], y])
    B = 5
    res = solver.bezier_fit(_dev(np.tile(q0, (B, 1))), _dev(np.tile(q1, (B, 1))), _dev(yy), _dev(off, torch.int64),
                            total_time=1.0, degree=20, ridge=0.0)
    torch.cuda.synchronize()
    one = solver.bezier_fit(q0[None], q1[None], y, np.array([0, 40]), total_time=1.0, degree=20, ridge=0.0)
    r = fc.to_numpy(res)
    assert list(r["status"]) == [0, 1, 0, 1, 0]
    for p in (0, 2, 4):
        assert np.array_equal(r["points"][p], one["points"][0]) and r["cost"][p] == one["cost"][0]
    assert np.isnan(r["cost"][1]) and np.isnan(r["cost"][3])
    # untouched: a second call into buffers of a known value
    fill = {k: torch.full_like(v, -7) for k, v in res.items()}
    from ikgrasp import _lib
    import ctypes as C
    prm = _lib.fit_params(20, 0.0, 1.0)
    a = [_dev(np.tile(q0, (B, 1))), _dev(np.tile(q1, (B, 1))), _dev(yy), _dev(off, torch.int64)]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(solver.lib.ikg_bezier_fit_batch(0, *[x.data_ptr() for x in a], B, 3, C.byref(prm),
                                               fill["points"].data_ptr(), fill["vpoints"].data_ptr(),
                                               fill["apoints"].data_ptr(), fill["cost"].data_ptr(),
                                               fill["status"].data_ptr(), s, 0))
    torch.cuda.synchronize()
    for p in (1, 3):
        for k in ("points", "vpoints", "apoints"):
            assert torch.all(fill[k][p] == -7), (k, p)
    assert np.array_equal(fill["points"][0].cpu().numpy(), one["points"][0])


def test_capture_and_replay(solver, d):
    import torch
    q0, q1, y, off = fc.ragged_inputs(d)
    a = (_dev(q0), _dev(q1), _dev(y), _dev(off, torch.int64))
    run = lambda: solver.bezier_fit(*a, total_time=1.0, degree=20, ridge=1e-10)
    direct = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run()
    for v in cap.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in direct:
        assert np.array_equal(cap[k].cpu().numpy(), direct[k].cpu().numpy()), k
    assert np.all(np.abs(cap["points"].cpu().numpy()).max(axis=(1, 2)) > 0)  # the replay wrote them after zero_()
    del graph


def test_empty_batch(solver):
    r = solver.bezier_fit(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(1, dtype=np.int64))
    assert r["points"].shape == (0, 21, 3) and r["cost"].shape == (0,)


# ---------------------------------------------------------------- one curve pair per state
def test_equal_curves_match_the_shared_rollout(solver, rd):
    fc.check_equal_curves_match_shared(solver, rd, ticks=8)


def test_distinct_curves_match_single_rollouts(solver, rd):
    fc.check_distinct_curves_match_single(solver, rd, ticks=8)


def test_per_state_rollout_with_device_tensors(solver, rd):
    back = lambda x: x.cpu().numpy()
    fc.check_distinct_curves_match_single(solver, rd, ticks=8, like=_dev, back=back)


def test_fit_then_track_against_the_rollout_oracle(solver, rd):
    fc.check_fit_then_track(solver.bezier_fit, solver, rd, "gpu")
