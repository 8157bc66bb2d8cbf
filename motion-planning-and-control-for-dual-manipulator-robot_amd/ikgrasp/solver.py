"""Batched solver front-end over the C-ABI.

`IKSolver` accepts either numpy arrays (host memory: the library stages them
through device scratch) or torch tensors already resident on a ROCm device
(device pointers, launched on torch's current stream — the zero-copy path the
benchmark uses).  The HIP kernel is the only compute path.
"""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass

import numpy as np

from . import _lib
from .model import GRAVITY, DualArmModel, load_nextage, load_nextage_inertia

_DT = {"f64": (_lib.IKG_F64, np.float64), "f32": (_lib.IKG_F32, np.float32)}


def _dtype(dtype):
    if dtype in ("f64", "float64", np.float64, "double"):
        return _DT["f64"]
    if dtype in ("f32", "float32", np.float32, "float"):
        return _DT["f32"]
    try:
        import torch
        if dtype == torch.float64:
            return _DT["f64"]
        if dtype == torch.float32:
            return _DT["f32"]
    except ImportError:  # pragma: no cover
        pass
    raise ValueError(f"unsupported dtype {dtype!r}")


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _q0_stride(shape, B: int, nq: int) -> int:
    """Row stride of a q0 array for ikg_solve_batch: [nq] or [1, nq] broadcast
    (stride 0), [B, nq] one row per target (stride nq).  Anything else would
    make the kernel read past the end of q0, so it is rejected here."""
    shape = tuple(shape)
    if shape == (nq,) or shape == (1, nq):
        return 0
    if shape == (B, nq):
        return nq
    raise ValueError(f"q0 must be [{nq}], [1,{nq}] or [{B},{nq}], got {list(shape)}")


@dataclass
class Solution:
    q: object            # [B, nq]
    converged: object    # [B] bool/uint8
    iters: object        # [B] int32
    err: object          # [B, 2] |log6| left/right at q
    best_seed: object = None


class IKSolver:
    """Owns one native model (`ikg_model_create`)."""

    def __init__(self, model: DualArmModel | None = None, device: int = 0, scene=None, specialize="auto"):
        """`scene`: an ikgrasp.collision.CollisionScene to attach (see set_collision).
        `specialize`: "auto" compiles model-specialised pair kernels
        (ikg_model_specialize) on a model's first solve per dtype and device
        unless the prebuilt library already has its specialisation (Nextage
        class); a failed compile warns and keeps the prebuilt generic kernel.
        True: always specialise, raising on failure.  False: prebuilt only."""
        if specialize not in ("auto", True, False):
            raise ValueError(f"specialize must be 'auto', True or False, got {specialize!r}")
        self._specialize = specialize
        self._specialized = set()
        self.lib = _lib.load()
        self.model = model if model is not None else load_nextage()
        self.desc = _lib.model_desc(self.model)
        h = C.c_void_p()
        _lib.check(self.lib.ikg_model_create(C.byref(self.desc), C.byref(h)))
        self._h = h
        self.device = device
        self.scene = None
        if scene is not None:
            self.set_collision(scene)
        self.inertias = None
        if model is None:  # the shipped Nextage tables come with the URDF's body inertias
            self.set_inertia(load_nextage_inertia())

    def set_collision(self, scene):
        """Attach the collision scene (ikg_model_set_collision); enables
        `check_collision=True` solves and `collision()` queries."""
        self._cdesc = _lib.collision_desc(scene)
        _lib.check(self.lib.ikg_model_set_collision(self._h, C.byref(self._cdesc)))
        self.scene = scene

    def set_inertia(self, inertias, gravity=GRAVITY):
        """Attach the body inertias (ikgrasp.model.BodyInertias, one per joint
        in q order) and the world-frame gravity (ikg_model_set_inertia);
        enables `dynamics()`."""
        if inertias.nq != self.nq:
            raise ValueError(f"inertias describe {inertias.nq} bodies, the model has {self.nq} joints")
        self._idesc = _lib.inertia_desc(inertias, gravity)
        _lib.check(self.lib.ikg_model_set_inertia(self._h, C.byref(self._idesc)))
        self.inertias = inertias
        self.gravity = tuple(float(x) for x in gravity)

    def _auto_specialize(self, device, code):
        if self._specialize is False or (device, code) in self._specialized:
            return
        self._specialized.add((device, code))
        flags = _lib.IKG_SPECIALIZE_IF_GENERIC if self._specialize == "auto" else 0
        rc = self.lib.ikg_model_specialize(self._h, device, code, flags)
        if rc != 0:
            msg = self.lib.ikg_last_error().decode()
            if self._specialize is True:
                raise _lib.IkgError(rc, msg)
            warnings.warn(f"model specialisation failed, using the prebuilt generic kernels: {msg}")

    def _native_solve(self, h, device, code, *rest):
        self._auto_specialize(device, code)
        return self.lib.ikg_solve_batch(h, device, code, *rest)

    def _native_multistart(self, h, device, code, *rest):
        self._auto_specialize(device, code)
        return self.lib.ikg_solve_multistart(h, device, code, *rest)

    def specialize(self, dtype="f64", device=None):
        """Compile the pair-layout kernels against this model's tables
        (ikg_model_specialize, hipRTC) for `dtype` on `device` (default: the
        solver's); later solves there use them.  Seconds for the first device."""
        code, _ = _dtype(dtype)
        _lib.check(self.lib.ikg_model_specialize(self._h, self.device if device is None else device, code, 0))

    def is_specialized(self, dtype="f64", device=None) -> bool:
        code, _ = _dtype(dtype)
        return bool(self.lib.ikg_model_is_specialized(self._h, self.device if device is None else device, code))

    def trim(self):
        """Give the scratch memory this model's pools keep for later solves
        back to the driver (ikg_model_trim); the solver stays usable."""
        _lib.check(self.lib.ikg_model_trim(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.ikg_model_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    @property
    def nq(self) -> int:
        return self.model.nq

    def params(self, eps=1e-3, dt=1e-2, max_iters=1000, lam=0.0, variant=_lib.IKG_VARIANT_AUTO, ppw=0,
               check_collision=False):
        """check_collision: reference `success` (converged AND collision-free,
        iterating on while converged-but-colliding, inverse_geometry.py:70)."""
        return _lib.default_params(eps=eps, dt=dt, max_iters=max_iters, lambda_=lam, variant=variant,
                                   problems_per_wave=ppw, check_collision=int(bool(check_collision)))

    # ------------------------------------------------------------------ batch
    def solve(self, targets, q0, dtype="f64", stream=None, **kw) -> Solution:
        """targets [B,12] cube placements; q0 [nq] (broadcast) or [B,nq]."""
        prm = self.params(**kw)
        if _is_torch(targets):
            return self._solve_torch(targets, q0, prm, stream)
        code, npt = _dtype(dtype)
        tg = np.ascontiguousarray(targets, dtype=npt).reshape(-1, 12)
        B = tg.shape[0]
        q = np.ascontiguousarray(q0, dtype=npt)
        stride = _q0_stride(q.shape, B, self.nq)
        q_out = np.empty((B, self.nq), dtype=npt)
        conv = np.empty(B, dtype=np.uint8)
        iters = np.empty(B, dtype=np.int32)
        err = np.empty((B, 2), dtype=npt)
        _lib.check(self._native_solve(
            self._h, self.device, code, tg.ctypes.data, q.ctypes.data, stride, B, C.byref(prm),
            q_out.ctypes.data, conv.ctypes.data, iters.ctypes.data, err.ctypes.data, None,
            _lib.IKG_FLAG_HOST_POINTERS))
        return Solution(q_out, conv.astype(bool), iters, err)

    def _solve_torch(self, targets, q0, prm, stream):
        import torch
        code, _ = _dtype(targets.dtype)
        if not targets.is_cuda:
            raise ValueError("torch targets must live on a ROCm device (or pass numpy arrays)")
        dev = targets.device
        tg = targets.contiguous().view(-1, 12)
        B = tg.shape[0]
        q = q0.to(device=dev, dtype=targets.dtype).contiguous()
        stride = _q0_stride(q.shape, B, self.nq)
        q_out = torch.empty((B, self.nq), dtype=targets.dtype, device=dev)
        conv = torch.empty(B, dtype=torch.uint8, device=dev)
        iters = torch.empty(B, dtype=torch.int32, device=dev)
        err = torch.empty((B, 2), dtype=targets.dtype, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self._native_solve(
            self._h, dev.index or 0, code, tg.data_ptr(), q.data_ptr(), stride, B, C.byref(prm),
            q_out.data_ptr(), conv.data_ptr(), iters.data_ptr(), err.data_ptr(), C.c_void_p(s), 0))
        return Solution(q_out, conv.bool(), iters, err)

    def _check_out(self, B, dtype_code, targets, q_out, conv, iters, err, best=None):
        """Preallocated torch buffers of the raw launches: shapes, dtypes and
        contiguity the kernels assume (a q_out narrower than nq would be
        written past its end)."""
        import torch
        fdt = torch.float64 if dtype_code == _lib.IKG_F64 else torch.float32
        want = [(targets, (B, 12), fdt, "targets"), (q_out, (B, self.nq), fdt, "q_out"),
                (conv, (B,), torch.uint8, "converged"), (iters, (B,), torch.int32, "iters"),
                (err, (B, 2), fdt, "err")]
        if best is not None:
            want.append((best, (B,), torch.int32, "best_seed"))
        for t, shape, dt, name in want:
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {list(shape)}, got "
                                 f"{t.dtype} {list(t.shape)}")
        for t, _, _, name in want:
            if not t.is_cuda:
                raise ValueError(f"{name} must be a device tensor")

    def solve_into(self, targets, q0, q_out, conv, iters, err, dtype_code, stream_handle, **kw):
        """Raw device-pointer launch (all tensors preallocated; used by bench.py)."""
        prm = self.params(**kw)
        self._check_out(targets.shape[0], dtype_code, targets, q_out, conv, iters, err)
        if not q0.is_contiguous() or q0.dtype != targets.dtype:
            raise ValueError("q0 must be contiguous and of the targets' dtype")
        stride = _q0_stride(q0.shape, targets.shape[0], self.nq)
        _lib.check(self._native_solve(
            self._h, targets.device.index or 0, dtype_code, targets.data_ptr(), q0.data_ptr(), stride,
            targets.shape[0], C.byref(prm), q_out.data_ptr(), conv.data_ptr(), iters.data_ptr(),
            err.data_ptr(), C.c_void_p(stream_handle), 0))

    def solve_multistart_into(self, targets, seeds, q_out, conv, iters, err, best, dtype_code, stream_handle, **kw):
        """Raw device-pointer multi-start launch (preallocated torch tensors; bench.py)."""
        prm = self.params(**kw)
        if seeds.dim() != 2 or seeds.shape[1] != self.nq:
            raise ValueError(f"seeds must be [S,{self.nq}], got {list(seeds.shape)}")
        if not seeds.is_contiguous() or seeds.dtype != targets.dtype:
            raise ValueError("seeds must be contiguous and of the targets' dtype")
        self._check_out(targets.shape[0], dtype_code, targets, q_out, conv, iters, err, best)
        _lib.check(self._native_multistart(
            self._h, targets.device.index or 0, dtype_code, targets.data_ptr(), targets.shape[0], seeds.data_ptr(),
            seeds.shape[0], C.byref(prm), q_out.data_ptr(), conv.data_ptr(), iters.data_ptr(), err.data_ptr(),
            best.data_ptr(), C.c_void_p(stream_handle), 0))

    # ------------------------------------------------------------------ multistart
    def solve_multistart(self, targets, seeds, dtype="f64", **kw) -> Solution:
        """S seeds x T targets -> best seed per target (ikg_solve_multistart)."""
        prm = self.params(**kw)
        code, npt = _dtype(dtype)
        tg = np.ascontiguousarray(targets, dtype=npt).reshape(-1, 12)
        sd = np.ascontiguousarray(seeds, dtype=npt).reshape(-1, self.nq)
        T, S = tg.shape[0], sd.shape[0]
        q_out = np.empty((T, self.nq), dtype=npt)
        conv = np.empty(T, dtype=np.uint8)
        iters = np.empty(T, dtype=np.int32)
        err = np.empty((T, 2), dtype=npt)
        best = np.empty(T, dtype=np.int32)
        _lib.check(self._native_multistart(
            self._h, self.device, code, tg.ctypes.data, T, sd.ctypes.data, S, C.byref(prm),
            q_out.ctypes.data, conv.ctypes.data, iters.ctypes.data, err.ctypes.data, best.ctypes.data, None,
            _lib.IKG_FLAG_HOST_POINTERS))
        return Solution(q_out, conv.astype(bool), iters, err, best)

    # ------------------------------------------------------------------ collision
    def collision(self, q, targets, dtype="f64"):
        """tools.collision(robot, q) with the cube at each target: q [B,nq],
        targets [B,12] -> bool [B] (numpy) or uint8 tensor (torch, device)."""
        if _is_torch(q):
            import torch
            code, _ = _dtype(q.dtype)
            qq = q.contiguous().view(-1, self.nq)
            tg = targets.to(device=q.device, dtype=q.dtype).contiguous().view(-1, 12)
            out = torch.empty(qq.shape[0], dtype=torch.uint8, device=q.device)
            s = torch.cuda.current_stream(q.device).cuda_stream
            _lib.check(self.lib.ikg_collision_batch(self._h, q.device.index or 0, code, qq.data_ptr(), tg.data_ptr(),
                                                    qq.shape[0], out.data_ptr(), C.c_void_p(s), 0))
            return out
        code, npt = _dtype(dtype)
        qq = np.ascontiguousarray(q, dtype=npt).reshape(-1, self.nq)
        tg = np.ascontiguousarray(np.broadcast_to(np.asarray(targets, dtype=npt).reshape(-1, 12), (qq.shape[0], 12)))
        out = np.empty(qq.shape[0], dtype=np.uint8)
        _lib.check(self.lib.ikg_collision_batch(self._h, self.device, code, qq.ctypes.data, tg.ctypes.data,
                                                qq.shape[0], out.ctypes.data, None, _lib.IKG_FLAG_HOST_POINTERS))
        return out.astype(bool)

    # ------------------------------------------------------------------ planner queries
    def distance(self, q, targets, pair_idx, dtype="f64") -> np.ndarray:
        """min over the listed active pairs of the pair distance (hpp-fcl
        computeDistance().min_distance; <= 0 when intersecting) for each
        configuration: q [B,nq], targets [B,12] (or one row, broadcast) -> [B]."""
        code, npt = _dtype(dtype)
        qq = np.ascontiguousarray(q, dtype=npt).reshape(-1, self.nq)
        tg = np.ascontiguousarray(np.broadcast_to(np.asarray(targets, dtype=npt).reshape(-1, 12), (qq.shape[0], 12)))
        idx = np.ascontiguousarray(pair_idx, dtype=np.int32).reshape(-1)
        out = np.empty(qq.shape[0], dtype=npt)
        _lib.check(self.lib.ikg_distance_batch(self._h, self.device, code, qq.ctypes.data, tg.ctypes.data,
                                               qq.shape[0], idx.ctypes.data, idx.size, out.ctypes.data, None,
                                               _lib.IKG_FLAG_HOST_POINTERS))
        return out

    def pair_distances(self, q, targets, pair_idx, dtype="f64") -> np.ndarray:
        """Each listed pair's distance: [B, len(pair_idx)] (one query per pair)."""
        return np.stack([self.distance(q, targets, [k], dtype) for k in pair_idx], axis=1)

    def target_env(self, targets, geoms, dtype="f64") -> np.ndarray:
        """The scene's target geometry at each placement [B,12] against the
        listed world-fixed geometries -> bool [B] (path.py:51-52)."""
        code, npt = _dtype(dtype)
        tg = np.ascontiguousarray(targets, dtype=npt).reshape(-1, 12)
        g = np.ascontiguousarray(geoms, dtype=np.int32).reshape(-1)
        out = np.empty(tg.shape[0], dtype=np.uint8)
        _lib.check(self.lib.ikg_target_env_batch(self._h, self.device, code, tg.ctypes.data, tg.shape[0],
                                                 g.ctypes.data, g.size, out.ctypes.data, None,
                                                 _lib.IKG_FLAG_HOST_POINTERS))
        return out.astype(bool)

    # ------------------------------------------------------------------ RRT-Connect planner primitives (fp64)
    def _i32_io(self, first):
        """(prep, empty) for int32 arrays of `first`'s kind (numpy, or tensors on its device)."""
        if _is_torch(first):
            import torch
            return (lambda x: x.to(device=first.device, dtype=torch.int32).contiguous().view(-1),
                    lambda *shape: torch.empty(shape, dtype=torch.int32, device=first.device))
        return (lambda x: np.ascontiguousarray(x, dtype=np.int32).reshape(-1),
                lambda *shape: np.empty(shape, dtype=np.int32))

    def se3_interpolate(self, A, B, alpha, stream=None):
        """ikg_se3_interpolate_batch: pin.SE3.Interpolate(A[c], B[c], alpha[c]) ->
        [C,12].  A, B [C,12], alpha [C] (numpy, or float64 ROCm tensors)."""
        prep, empty, ptr, s, device, flags = self._f64_io(A, stream)
        aa, bb, al = prep(A, 12), prep(B, 12), prep(alpha, 1)
        n = aa.shape[0]
        if bb.shape[0] != n or al.shape[0] != n:
            raise ValueError(f"A has {n} rows: B and alpha need as many")
        out = empty(n, 12)
        _lib.check(self.lib.ikg_se3_interpolate_batch(device, ptr(aa), ptr(bb), ptr(al), n, ptr(out), s, flags))
        return out

    def nearest(self, nodes, counts, queries, stream=None):
        """ikg_nearest_batch: per tree the nearest row to its query, the lowest
        index among exact ties -> (index [P] int32, dist [P]).  nodes
        [P,cap,nq] (any row length nq), counts [P], queries [P,nq] (numpy, or
        ROCm tensors: float64 and int32); counts[p] == 0 gives index -1."""
        if nodes.ndim != 3:
            raise ValueError(f"nodes must be [P, cap, nq], got {list(nodes.shape)}")
        P, cap, nq = (int(x) for x in nodes.shape)
        prep, empty, ptr, s, device, flags = self._f64_io(nodes, stream)
        iprep, iempty = self._i32_io(nodes)
        nn, qq, cc = prep(nodes, nq), prep(queries, nq), iprep(counts)
        if qq.shape[0] != P or cc.shape[0] != P:
            raise ValueError(f"nodes hold {P} trees: queries and counts need as many rows")
        index, dist = iempty(P), empty(P)
        _lib.check(self.lib.ikg_nearest_batch(device, ptr(nn), cap, ptr(cc), ptr(qq), nq, P, ptr(index), ptr(dist), s,
                                              flags))
        return index, dist

    def project_paths(self, q_curr, cube_curr, cube_rand, step_size=0.025, max_nodes=64, geoms=None, stream=None,
                      **kw) -> dict:
        """ikg_project_paths: path.py:125-163 for C chains, the whole loop on
        the device.  q_curr [C,nq], cube_curr, cube_rand [C,12] (numpy, or
        float64 ROCm tensors: then nothing waits on the host).  geoms: the
        world-fixed geometries of the placement check (default: the scene's
        table and obstacle).  `kw`: the solve's parameters (default: the
        planner's check_collision=True).  -> dict of robot_path
        [C,max_nodes,nq], cube_path [C,max_nodes,12], n_nodes [C], status [C]
        (0 reached, 1 placement collision, 2 failed IK, 3 cut at max_nodes)."""
        if self.scene is None:
            raise RuntimeError("project_paths needs a collision scene (set_collision)")
        kw.setdefault("check_collision", True)
        prm = self.params(**kw)
        nq = self.nq
        prep, empty, ptr, s, device, flags = self._f64_io(q_curr, stream)
        _, iempty = self._i32_io(q_curr)
        qq, ca, cb = prep(q_curr, nq), prep(cube_curr, 12), prep(cube_rand, 12)
        n = qq.shape[0]
        if ca.shape[0] != n or cb.shape[0] != n:
            raise ValueError(f"q_curr has {n} rows: cube_curr and cube_rand need as many")
        g = np.ascontiguousarray(self.scene.env_geoms() if geoms is None else geoms, dtype=np.int32).reshape(-1)
        M = int(max_nodes)
        res = {"robot_path": empty(n, M, nq), "cube_path": empty(n, M, 12), "n_nodes": iempty(n), "status": iempty(n)}
        self._auto_specialize(device, _lib.IKG_F64)
        _lib.check(self.lib.ikg_project_paths(self._h, device, ptr(qq), ptr(ca), ptr(cb), n, float(step_size), M,
                                              g.ctypes.data, g.size, C.byref(prm), ptr(res["robot_path"]),
                                              ptr(res["cube_path"]), ptr(res["n_nodes"]), ptr(res["status"]), s, flags))
        return res

    # ------------------------------------------------------------------ trajectory check (fp64)
    def check_curves(self, points, t_min, t_max, mult=1.0, samples=151, cube="carried", pair_idx=None,
                     per_sample=False, samples_per_wave=0, stream=None) -> dict:
        """ikg_trajectory_check_batch: B joint-space Bezier curves sampled at
        `samples` times each, one verdict per curve.  points [B, n_points, nq]
        (numpy, or a float64 ROCm tensor); cube "carried" (the placement at
        which the left hand's grasp error is zero) or fixed placements [B,12]
        (one row is broadcast).  pair_idx: the scene pairs of the clearance
        (None = scene.obstacle_pairs(); empty = no clearance).  -> dict of
        first_collision, first_pair, n_collision, min_clearance, arg_clearance,
        max_grasp, arg_grasp, max_limit, arg_limit [B]; with per_sample also
        collision, clearance, grasp, limit [B,S] and cube [B,S,12]."""
        if self.scene is None:
            raise RuntimeError("check_curves needs a collision scene (set_collision)")
        if not _is_torch(points):
            points = np.asarray(points, dtype=np.float64)
        if points.ndim != 3 or points.shape[2] != self.nq:
            raise ValueError(f"points must be [B, n_points, {self.nq}], got {list(points.shape)}")
        B, n_points = int(points.shape[0]), int(points.shape[1])
        S = int(samples)
        prep, empty, ptr, s, device, flags = self._f64_io(points, stream)
        flat = prep(points, n_points * self.nq)
        fixed = None
        if not isinstance(cube, str):
            if _is_torch(points) != _is_torch(cube):
                raise ValueError("fixed cube placements must be the same kind of array as points "
                                 "(numpy, or a float64 tensor on the points' device)")
            fixed = prep(cube, 12)
            if fixed.shape[0] == 1 and B != 1:
                fixed = fixed.expand(B, 12).contiguous() if _is_torch(fixed) else np.ascontiguousarray(
                    np.broadcast_to(fixed, (B, 12)))
            if fixed.shape[0] != B:
                raise ValueError(f"cube has {fixed.shape[0]} placements, points hold {B} curves")
        elif cube != "carried":
            raise ValueError(f"cube must be 'carried' or placements [B,12], got {cube!r}")
        idx = np.ascontiguousarray(self.scene.obstacle_pairs() if pair_idx is None else pair_idx,
                                   dtype=np.int32).reshape(-1)
        prm = _lib.trajcheck_params(S, _lib.CUBE_CARRIED if fixed is None else _lib.CUBE_FIXED, samples_per_wave)
        if _is_torch(points):
            import torch
            kinds = {np.int32: torch.int32, np.float64: torch.float64, np.uint8: torch.uint8}
            alloc = lambda t, *shape: torch.empty(shape, dtype=kinds[t], device=points.device)
        else:
            alloc = lambda t, *shape: np.empty(shape, dtype=t)
        res = {name: alloc(t, B) for name, t in _lib.TRAJCHECK_CURVE}
        if per_sample:
            res.update({name: alloc(t, B, S, *tail) for name, t, tail in _lib.TRAJCHECK_SAMPLE})
        bset = _lib.BezierSet(ptr(flat), n_points, float(t_min), float(t_max), float(mult))
        out = _lib.TrajCheckOut(*[ptr(res.get(f[0])) for f in _lib.TRAJCHECK_CURVE + _lib.TRAJCHECK_SAMPLE])
        _lib.check(self.lib.ikg_trajectory_check_batch(self._h, device, C.byref(bset), B, ptr(fixed),
                                                       idx.ctypes.data if idx.size else None, idx.size, C.byref(prm),
                                                       C.byref(out), s, flags))
        return res

    # ------------------------------------------------------------------ trajectory dynamics (fp64)
    def curve_dynamics(self, points, t_min, t_max, mult=1.0, samples=151, velocity=None, effort=None,
                       per_sample=False, samples_per_wave=0, stream=None) -> dict:
        """ikg_trajectory_dynamics_batch: inverse dynamics at `samples` times
        along B joint-space Bezier curves and the actuator-limit ratios folded
        per curve.  points [B, n_points, nq] (numpy, or a float64 ROCm tensor),
        n_points 5 .. 64; velocity, effort: the joints' limits ([nq], one
        number, or None / np.inf = unlimited).  -> dict of speed_scale,
        torque_use, static_use, torque_scale [B], n_static [B] and arg_speed,
        arg_torque_use, arg_static, arg_torque_scale [B,2] = (sample, joint);
        with per_sample also tau, g [B,S,nq].  A duration s (t_max - t_min)
        meets every limit iff n_static == 0 and s >= max(speed_scale,
        torque_scale).  Needs `set_inertia`."""
        if not _is_torch(points):
            points = np.asarray(points, dtype=np.float64)
        if points.ndim != 3 or points.shape[2] != self.nq:
            raise ValueError(f"points must be [B, n_points, {self.nq}], got {list(points.shape)}")
        B, n_points = int(points.shape[0]), int(points.shape[1])
        S = int(samples)
        prm = _lib.trajdyn_params(self.nq, S, velocity, effort, samples_per_wave)
        prep, empty, ptr, s, device, flags = self._f64_io(points, stream)
        flat = prep(points, n_points * self.nq)
        if _is_torch(points):
            import torch
            kinds = {np.int32: torch.int32, np.float64: torch.float64}
            alloc = lambda t, *shape: torch.empty(shape, dtype=kinds[t], device=points.device)
        else:
            alloc = lambda t, *shape: np.empty(shape, dtype=t)
        res = {name: alloc(t, B, *tail) for name, t, tail in _lib.TRAJDYN_CURVE}
        if per_sample:
            res.update({name: alloc(np.float64, B, S, self.nq) for name in _lib.TRAJDYN_SAMPLE})
        bset = _lib.BezierSet(ptr(flat), n_points, float(t_min), float(t_max), float(mult))
        out = _lib.TrajDynOut(*[ptr(res.get(f[0])) for f in _lib.TRAJDYN_CURVE],
                              *[ptr(res.get(name)) for name in _lib.TRAJDYN_SAMPLE])
        _lib.check(self.lib.ikg_trajectory_dynamics_batch(self._h, device, C.byref(bset), B, C.byref(prm),
                                                          C.byref(out), s, flags))
        return res

    # ------------------------------------------------------------------ log6
    def log6(self, M, dtype="f64") -> np.ndarray:
        """pin.log6 of placements [B,12] -> [B,6] ([v; w])."""
        code, npt = _dtype(dtype)
        mm = np.ascontiguousarray(M, dtype=npt).reshape(-1, 12)
        out = np.empty((mm.shape[0], 6), dtype=npt)
        _lib.check(self.lib.ikg_log6_batch(self.device, code, mm.ctypes.data, mm.shape[0], out.ctypes.data, None,
                                           _lib.IKG_FLAG_HOST_POINTERS))
        return out

    # ------------------------------------------------------------------ FK
    def fk(self, q, dtype="f64") -> np.ndarray:
        """Hands placements [B, 2, 12] (R row-major, t) for q [B, nq]."""
        code, npt = _dtype(dtype)
        qq = np.ascontiguousarray(q, dtype=npt).reshape(-1, self.nq)
        out = np.empty((qq.shape[0], 2, 12), dtype=npt)
        _lib.check(self.lib.ikg_fk_batch(self._h, self.device, code, qq.ctypes.data, qq.shape[0],
                                         out.ctypes.data, None, _lib.IKG_FLAG_HOST_POINTERS))
        return out

    # ------------------------------------------------------------------ controller kinematics
    FRAME_KIN_OUTPUTS = ("placement", "velocity", "J", "dJ", "dJv", "err", "derr")

    def frame_kinematics(self, q, v=None, q_des=None, v_des=None, rf=_lib.IKG_LOCAL_WORLD_ALIGNED,
                         outputs=("placement", "velocity", "J", "dJ", "dJv"), dtype="f64", stream=None) -> dict:
        """ikg_frame_kinematics_batch: per state and hand (LARM_EFF, RARM_EFF)
        the kinematic terms of control.py:284-345 in reference frame `rf`.
        q, v [B,nq] (numpy, or torch tensors on a ROCm device); q_des / v_des
        only for 'err' / 'derr'.  Returns {name: array} with placement [B,2,12],
        velocity [B,2,6], J / dJ [B,12,nq], dJv / err / derr [B,12]."""
        unknown = set(outputs) - set(self.FRAME_KIN_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        nq = self.nq
        shapes = {"placement": (2, 12), "velocity": (2, 6), "J": (12, nq), "dJ": (12, nq), "dJv": (12,),
                  "err": (12,), "derr": (12,)}
        if ("err" in outputs or "derr" in outputs) and q_des is None:
            raise ValueError("err/derr need q_des")
        if _is_torch(q):
            import torch
            code, _ = _dtype(q.dtype)
            dev = q.device
            prep = lambda x: None if x is None else x.to(device=dev, dtype=q.dtype).contiguous().view(-1, nq)
            qq, vv, qd, vd = prep(q), prep(v), prep(q_des), prep(v_des)
            B = qq.shape[0]
            for name, x in (("v", vv), ("q_des", qd), ("v_des", vd)):
                if x is not None and x.shape[0] != B:
                    raise ValueError(f"{name} has {x.shape[0]} rows, q has {B}")
            res = {k: torch.empty((B,) + shapes[k], dtype=q.dtype, device=dev) for k in outputs}
            ptr = lambda x: None if x is None else x.data_ptr()
            out = _lib.FrameKinOut(*[ptr(res.get(k)) for k in self.FRAME_KIN_OUTPUTS])
            s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
            _lib.check(self.lib.ikg_frame_kinematics_batch(
                self._h, dev.index or 0, code, ptr(qq), ptr(vv), ptr(qd), ptr(vd), B, int(rf), C.byref(out),
                C.c_void_p(s), 0))
            return res
        code, npt = _dtype(dtype)
        prep = lambda x: None if x is None else np.ascontiguousarray(x, dtype=npt).reshape(-1, nq)
        qq, vv, qd, vd = prep(q), prep(v), prep(q_des), prep(v_des)
        B = qq.shape[0]
        for name, x in (("v", vv), ("q_des", qd), ("v_des", vd)):
            if x is not None and x.shape[0] != B:
                raise ValueError(f"{name} has {x.shape[0]} rows, q has {B}")
        res = {k: np.empty((B,) + shapes[k], dtype=npt) for k in outputs}
        ptr = lambda x: None if x is None else x.ctypes.data
        out = _lib.FrameKinOut(*[ptr(res.get(k)) for k in self.FRAME_KIN_OUTPUTS])
        _lib.check(self.lib.ikg_frame_kinematics_batch(
            self._h, self.device, code, ptr(qq), ptr(vv), ptr(qd), ptr(vd), B, int(rf), C.byref(out), None,
            _lib.IKG_FLAG_HOST_POINTERS))
        return res

    # ------------------------------------------------------------------ controller dynamics (control.py:284-286)
    DYNAMICS_OUTPUTS = ("M", "nle", "g")

    def dynamics(self, q, v=None, outputs=("M", "nle"), dtype="f64", stream=None) -> dict:
        """ikg_dynamics_batch: per state the joint-space inertia matrix
        M [B,nq,nq] (data.M of pin.computeAllTerms, both triangles), the
        non-linear effects nle [B,nq] (pin.nonLinearEffects) and g [B,nq] (nle
        at zero velocity).  q, v [B,nq] (numpy, or torch tensors on a ROCm
        device); v None = zero velocity.  Needs `set_inertia`."""
        unknown = set(outputs) - set(self.DYNAMICS_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        nq = self.nq
        shapes = {"M": (nq, nq), "nle": (nq,), "g": (nq,)}
        if _is_torch(q):
            import torch
            code, _ = _dtype(q.dtype)
            dev = q.device
            if not q.is_cuda:
                raise ValueError("torch inputs must live on a ROCm device (or pass numpy arrays)")
            prep = lambda x: None if x is None else x.to(device=dev, dtype=q.dtype).contiguous().view(-1, nq)
            qq, vv = prep(q), prep(v)
            B = qq.shape[0]
            if vv is not None and vv.shape[0] != B:
                raise ValueError(f"v has {vv.shape[0]} rows, q has {B}")
            res = {k: torch.empty((B,) + shapes[k], dtype=q.dtype, device=dev) for k in outputs}
            ptr = lambda x: None if x is None else x.data_ptr()
            out = _lib.DynamicsOut(*[ptr(res.get(k)) for k in self.DYNAMICS_OUTPUTS])
            s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
            _lib.check(self.lib.ikg_dynamics_batch(self._h, dev.index or 0, code, ptr(qq), ptr(vv), B, C.byref(out),
                                                   C.c_void_p(s), 0))
            return res
        code, npt = _dtype(dtype)
        prep = lambda x: None if x is None else np.ascontiguousarray(x, dtype=npt).reshape(-1, nq)
        qq, vv = prep(q), prep(v)
        B = qq.shape[0]
        if vv is not None and vv.shape[0] != B:
            raise ValueError(f"v has {vv.shape[0]} rows, q has {B}")
        res = {k: np.empty((B,) + shapes[k], dtype=npt) for k in outputs}
        ptr = lambda x: None if x is None else x.ctypes.data
        out = _lib.DynamicsOut(*[ptr(res.get(k)) for k in self.DYNAMICS_OUTPUTS])
        _lib.check(self.lib.ikg_dynamics_batch(self._h, self.device, code, ptr(qq), ptr(vv), B, C.byref(out), None,
                                               _lib.IKG_FLAG_HOST_POINTERS))
        return res

    # ------------------------------------------------------------------ controller torques (control.py:284-406)
    CONTROL_OUTPUTS = ("tau", "qdd", "xdd", "Lambda", "fc")

    def control_torques(self, q, v, q_des, v_des, outputs=CONTROL_OUTPUTS, stream=None, **gains) -> dict:
        """ikg_control_torque_batch (fp64): per state the controller's torques
        tau [B,nq] (what sim.step receives), the QP's solution qdd [B,nq],
        xdd [B,12] (x_ddot_des_total), Lambda [B,2,36] and fc [B,12] (before the
        bias).  q, v, q_des, v_des [B,nq] (numpy, or float64 torch tensors on a
        ROCm device; v / v_des None = zero).  `gains`: Kp, Kv, Kf, Kt,
        lambda_reg, qp_reg, fc_bias, zero_tau (defaults: the reference's)."""
        unknown = set(outputs) - set(self.CONTROL_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        nq = self.nq
        prm = _lib.control_params(**gains)
        shapes = {"tau": (nq,), "qdd": (nq,), "xdd": (12,), "Lambda": (2, 36), "fc": (12,)}
        if _is_torch(q):
            import torch
            if not q.is_cuda or q.dtype != torch.float64:
                raise ValueError("torch inputs must be float64 tensors on a ROCm device (or pass numpy arrays)")
            dev = q.device
            prep = lambda x: None if x is None else x.to(device=dev, dtype=torch.float64).contiguous().view(-1, nq)
            arrs = [prep(x) for x in (q, v, q_des, v_des)]
            empty = lambda B, k: torch.empty((B,) + shapes[k], dtype=torch.float64, device=dev)
            ptr = lambda x: None if x is None else x.data_ptr()
            s = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
            device, flags = dev.index or 0, 0
        else:
            prep = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1, nq)
            arrs = [prep(x) for x in (q, v, q_des, v_des)]
            empty = lambda B, k: np.empty((B,) + shapes[k], dtype=np.float64)
            ptr = lambda x: None if x is None else x.ctypes.data
            s, device, flags = None, self.device, _lib.IKG_FLAG_HOST_POINTERS
        if arrs[2] is None:
            raise ValueError("q_des is required")
        B = arrs[0].shape[0]
        for name, x in zip(("v", "q_des", "v_des"), arrs[1:]):
            if x is not None and x.shape[0] != B:
                raise ValueError(f"{name} has {x.shape[0]} rows, q has {B}")
        res = {k: empty(B, k) for k in outputs}
        out = _lib.ControlOut(*[ptr(res.get(k)) for k in self.CONTROL_OUTPUTS])
        _lib.check(self.lib.ikg_control_torque_batch(self._h, device, *[ptr(x) for x in arrs], B, C.byref(prm),
                                                     C.byref(out), s, flags))
        return res

    # ------------------------------------------------------------------ forward dynamics, curves, closed-loop rollout
    def _f64_io(self, first, stream):
        """(prep, empty, ptr, stream, device, flags) for float64 numpy arrays or ROCm torch tensors."""
        if _is_torch(first):
            import torch
            if not first.is_cuda or first.dtype != torch.float64:
                raise ValueError("torch inputs must be float64 tensors on a ROCm device (or pass numpy arrays)")
            dev = first.device
            prep = lambda x, w: None if x is None else x.to(device=dev, dtype=torch.float64).contiguous().view(-1, w)
            empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
            ptr = lambda x: None if x is None else x.data_ptr()
            s = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
            return prep, empty, ptr, s, dev.index or 0, 0
        prep = lambda x, w: None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1, w)
        empty = lambda *shape: np.empty(shape, dtype=np.float64)
        ptr = lambda x: None if x is None else x.ctypes.data
        return prep, empty, ptr, None, self.device, _lib.IKG_FLAG_HOST_POINTERS

    def forward_dynamics(self, q, v, tau, stream=None):
        """ikg_forward_dynamics_batch (fp64): qdd [B,nq] = M(q)^-1 (tau - nle(q, v)),
        pin.aba.  q, v, tau [B,nq] (numpy, or float64 torch tensors on a ROCm
        device; v None = zero).  Needs `set_inertia`."""
        nq = self.nq
        prep, empty, ptr, s, device, flags = self._f64_io(q, stream)
        qq, vv, tt = prep(q, nq), prep(v, nq), prep(tau, nq)
        B = qq.shape[0]
        for name, x in (("v", vv), ("tau", tt)):
            if x is not None and x.shape[0] != B:
                raise ValueError(f"{name} has {x.shape[0]} rows, q has {B}")
        if tt is None:
            raise ValueError("tau is required")
        out = empty(B, nq)
        _lib.check(self.lib.ikg_forward_dynamics_batch(self._h, device, ptr(qq), ptr(vv), ptr(tt), B, ptr(out), s,
                                                       flags))
        return out

    def bezier(self, points, t_min, t_max, mult, times, stream=None):
        """ikg_bezier_eval_batch: the reference's Bezier(points, t_min, t_max,
        mult)(t) for every t of `times` [K] -> [K, dim].  points [n, dim] is a
        host array; times numpy or a float64 ROCm tensor.  A time outside
        [t_min, t_max] raises for numpy times, as the reference does."""
        pts, t_min, t_max, mult = _lib.curve((points, t_min, t_max, mult))
        prep, empty, ptr, s, device, flags = self._f64_io(times, stream)
        tt = prep(times, 1)
        K = tt.shape[0]
        out = empty(K, pts.shape[1])
        _lib.check(self.lib.ikg_bezier_eval_batch(device, pts.ctypes.data, pts.shape[0], pts.shape[1], t_min, t_max,
                                                  mult, ptr(tt), K, ptr(out), s, flags))
        return out

    ROLLOUT_OUTPUTS = ("q", "v", "t", "q_hist", "v_hist", "tau_hist")

    def bezier_fit(self, q0, q1, path_points, offsets, total_time=1.0, degree=20, ridge=0.0, derivatives=True,
                   stream=None) -> dict:
        """ikg_bezier_fit_batch on this solver's device: see the module's `bezier_fit`."""
        return bezier_fit(q0, q1, path_points, offsets, total_time=total_time, degree=degree, ridge=ridge,
                          derivatives=derivatives, device=self.device, stream=stream)

    def rollout(self, q0, v0, trajs, t0=None, ticks=0, dt_sim=1e-3, dt_traj=1e-2, record_every=0,
                outputs=("q", "v", "t"), stream=None, per_state=False, **gains) -> dict:
        """ikg_control_rollout (fp64): `ticks` closed-loop ticks of B states in
        one call: desired state from the curves, the torque law, forward
        dynamics, semi-implicit Euler, clock.  The plant is the free rigid-body
        tree (no contact, cube, joint limits or damping).
        q0, v0 [B,nq] (numpy or float64 ROCm tensors, never written; v0 None =
        zero); t0 [B] or None = the q curve's t_min.  trajs = (q curve, v curve),
        each an object with the reference Bezier's control_points_, T_min_,
        T_max_, mult_T_ or a (points, t_min, t_max, mult) tuple.  dt_traj: the
        trajectory clock's step per tick (the reference's DT = 0.01 per 1 ms
        tick).  outputs: final q, v [B,nq], t [B]; with record_every > 0
        q_hist, v_hist, tau_hist [B, ticks // record_every, nq].
        `gains` as control_torques.
        per_state=True (ikg_control_rollout_curves): state p follows its own
        curve pair; trajs = ((points [B,n,nq], t_min, t_max, mult), (vpoints
        [B,n',nq], t_min, t_max, mult)) with arrays of q0's kind (numpy, or
        float64 tensors on q0's device).  B equal curves give the shared-curve
        result bit for bit."""
        unknown = set(outputs) - set(self.ROLLOUT_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        nq = self.nq
        prm = _lib.rollout_params(ticks, dt_sim, dt_traj, record_every, **gains)
        prep, empty, ptr, s, device, flags = self._f64_io(q0, stream)
        qq, vv = prep(q0, nq), prep(v0, nq)
        tt = None if t0 is None else prep(t0, 1)
        B = qq.shape[0]
        if per_state:
            sets, keep = [], []
            for name, (pts, t_min, t_max, mult) in zip(("q", "v"), trajs):
                if _is_torch(pts) != _is_torch(qq):
                    raise ValueError(f"the {name} curves must be the same kind of array as q0")
                if pts.ndim != 3 or pts.shape[0] != B or pts.shape[2] != nq:
                    raise ValueError(f"the {name} curves must be [{B}, n_points, {nq}], got {list(pts.shape)}")
                n_points = int(pts.shape[1])
                flat = prep(pts, n_points * nq)
                keep.append(flat)
                sets.append(_lib.BezierSet(ptr(flat), n_points, float(t_min), float(t_max), float(mult)))
            entry, bq, bv = self.lib.ikg_control_rollout_curves, sets[0], sets[1]
        else:
            bq, keep_q = _lib.bezier_desc(trajs[0], nq)
            bv, keep_v = _lib.bezier_desc(trajs[1], nq)
            keep = (keep_q, keep_v)
            entry = self.lib.ikg_control_rollout
        if vv is not None and vv.shape[0] != B:
            raise ValueError(f"v0 has {vv.shape[0]} rows, q0 has {B}")
        if tt is not None and tt.shape[0] != B:
            raise ValueError(f"t0 has {tt.shape[0]} entries, q0 has {B} rows")
        R = int(ticks) // int(record_every) if record_every else 0
        if not R and any(k.endswith("_hist") for k in outputs):
            raise ValueError("history outputs need record_every > 0 and ticks >= record_every")
        shape = lambda k: (B,) if k == "t" else ((B, R, nq) if k.endswith("_hist") else (B, nq))
        res = {k: empty(*shape(k)) for k in outputs}
        out = _lib.RolloutOut(*[ptr(res.get(k)) for k in self.ROLLOUT_OUTPUTS])
        _lib.check(entry(self._h, device, ptr(qq), ptr(vv), ptr(tt), B, C.byref(bq), C.byref(bv), C.byref(prm),
                         C.byref(out), s, flags))
        del keep
        return res


def bezier_fit(q0, q1, path_points, offsets, total_time=1.0, degree=20, ridge=0.0, derivatives=True, device=0,
               stream=None) -> dict:
    """ikg_bezier_fit_batch (fp64): the reference's maketraj (control.py:63-197)
    for B paths in one launch, solved exactly (Householder least squares on the
    degree - 5 control points its constraints leave free).
    q0, q1 [B,dim]; path_points packed [offsets[B],dim]; offsets [B+1] int64,
    offsets[0] = 0.  All numpy, or all ROCm tensors (float64, offsets int64):
    then nothing leaves the device and no limit but the parameters' is checked
    on the host; a path whose count is out of range gets status 1, cost NaN.
    -> dict of points [B,degree+1,dim], cost [B], status [B] (int32) and, with
    `derivatives`, vpoints [B,degree,dim], apoints [B,degree-1,dim]: the
    unscaled derivative control points (Bezier.derivative's, without its
    1 / total_time multiplier).  No model is involved."""
    lib = _lib.load()
    prm = _lib.fit_params(degree, ridge, total_time)
    d = int(degree)
    if _is_torch(q0):
        import torch
        dev = q0.device
        if not q0.is_cuda or q0.dtype != torch.float64:
            raise ValueError("torch inputs must be float64 tensors on a ROCm device (or pass numpy arrays)")
        if not (_is_torch(offsets) and offsets.is_cuda and offsets.dtype == torch.int64):
            raise ValueError("with tensor inputs offsets must be an int64 tensor on the same device")
        dim = int(q0.shape[-1])
        a0, a1 = q0.contiguous().view(-1, dim), q1.to(device=dev, dtype=torch.float64).contiguous().view(-1, dim)
        yy = path_points.to(device=dev, dtype=torch.float64).contiguous().view(-1, dim)
        off = offsets.contiguous()
        empty = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
        i32 = torch.int32
        ptr = lambda x: None if x is None else x.data_ptr()
        s = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
        device, flags = dev.index or 0, 0
    else:
        a0 = np.ascontiguousarray(q0, dtype=np.float64)
        dim = int(a0.shape[-1])
        a0 = a0.reshape(-1, dim)
        a1 = np.ascontiguousarray(q1, dtype=np.float64).reshape(-1, dim)
        yy = np.ascontiguousarray(path_points, dtype=np.float64).reshape(-1, dim)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(off) and int(off[-1]) != len(yy):
            raise ValueError(f"offsets end at {int(off[-1])}, path_points has {len(yy)} rows")
        empty = lambda *shape, dtype=np.float64: np.empty(shape, dtype=dtype)
        i32 = np.int32
        ptr = lambda x: None if x is None else x.ctypes.data
        s, flags = None, _lib.IKG_FLAG_HOST_POINTERS
    B = a0.shape[0]
    if a1.shape[0] != B or off.shape[0] != B + 1:
        raise ValueError(f"q0 has {B} rows: q1 needs {B} and offsets {B + 1} entries")
    if not 6 <= d <= 20:
        raise ValueError("degree must be in [6, 20]")
    res = {"points": empty(B, d + 1, dim), "cost": empty(B), "status": empty(B, dtype=i32)}
    if derivatives:
        res["vpoints"], res["apoints"] = empty(B, d, dim), empty(B, d - 1, dim)
    _lib.check(lib.ikg_bezier_fit_batch(device, ptr(a0), ptr(a1), ptr(yy), ptr(off), B, dim, C.byref(prm),
                                        ptr(res["points"]), ptr(res.get("vpoints")), ptr(res.get("apoints")),
                                        ptr(res["cost"]), ptr(res["status"]), s, flags))
    return res
