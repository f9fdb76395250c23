"""Batched solver API over the C ABI (libmav_trajectory_generation.so).

Arrays may be numpy arrays (host; the library stages them through HBM) or
torch CUDA tensors (device-resident; launched on torch's current stream so
torch.cuda.Event timing and stream ordering work).  There is no CPU path.

Layouts follow include/mtg.h:
  values [B][K+1][N/2][D] float64, mask [B][K+1] uint8, times [B][K] float64
  coeffs [B][K][D][N], free [B][D][(K+1)*N/2], n_free [B], cost [B], status [B]
"""
import ctypes

import numpy as np

from . import _native as nat


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _addr(x):
    if x is None:
        return None
    if _is_torch(x):
        return x.data_ptr()
    return x.ctypes.data


# struct mtg_extremum (include/mtg.h)
EXTREMUM_DTYPE = np.dtype([("time", "<f8"), ("value", "<f8"), ("segment", "<i4"), ("reserved", "<i4")])


class Context:
    """Owns one mtg_ctx (a HIP stream + staging buffers on one device)."""

    def __init__(self, device=0):
        self._lib = nat.load()
        h = ctypes.c_void_p()
        nat.check(self._lib.mtg_create(device, ctypes.byref(h)))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            self._lib.mtg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_handle):
        """Launch on this hipStream_t (an int, e.g. torch.cuda.current_stream().cuda_stream);
        0 / None is the HIP null stream (torch's default stream)."""
        nat.check(self._lib.mtg_set_stream(self.handle, stream_handle or None), self.handle)

    def reset_stream(self):
        """Launch on the context's own stream again."""
        nat.check(self._lib.mtg_reset_stream(self.handle), self.handle)

    def synchronize(self):
        nat.check(self._lib.mtg_synchronize(self.handle), self.handle)

    def last_kernel_ms(self):
        ms = ctypes.c_float(0)
        nat.check(self._lib.mtg_last_kernel_ms(self.handle, ctypes.byref(ms)), self.handle)
        return ms.value

    def enable_timing(self, ring):
        """Record a HIP event pair around each of the last `ring` kernel launches."""
        nat.check(self._lib.mtg_enable_timing(self.handle, ring), self.handle)

    def kernel_times_ms(self, n):
        """Durations (ms) of up to n most recent launches, oldest first (synchronizes)."""
        buf = (ctypes.c_float * max(n, 1))()
        got = ctypes.c_int(0)
        nat.check(self._lib.mtg_kernel_times(self.handle, buf, n, ctypes.byref(got)), self.handle)
        return np.array(buf[:got.value], dtype=np.float64)

    def solve_call(self, N, r, values, mask, times, coeffs, free=None, n_free=None, cost=None, status=None,
                   split=False, general=False, dl=False, column=False):
        """A zero-argument callable that launches one device-pointer solve asynchronously on the
        current stream with the arguments bound once (the bench's step; minimal host overhead)."""
        import torch
        B, V, h, D = values.shape
        K = V - 1
        self.set_stream(torch.cuda.current_stream(values.device).cuda_stream)
        flags = nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC | (nat.MTG_FLAG_SPLIT_KERNELS if split else 0)
        flags |= nat.MTG_FLAG_GENERAL_KERNEL if general else 0
        flags |= nat.MTG_FLAG_DL_KERNEL if dl else 0
        flags |= nat.MTG_FLAG_COLUMN_KERNEL if column else 0
        fn = self._lib.mtg_solve_linear_batch
        args = (self.handle, N, D, K, r, B, _addr(values), _addr(mask), _addr(times), _addr(coeffs), _addr(free),
                _addr(n_free), _addr(cost), _addr(status), flags)
        handle = self.handle

        def call():
            rc = fn(*args)
            if rc:
                nat.check(rc, handle)
        return call

    def cost_call(self, N, r, vertex_values, times, scales, cost):
        """Zero-argument callable: one asynchronous device-pointer mtg_cost_at_times_batch launch on
        torch's current stream (the config-5 bench step)."""
        import torch
        B, V, h, D = vertex_values.shape
        C = scales.shape[0]
        self.set_stream(torch.cuda.current_stream(vertex_values.device).cuda_stream)
        fn = self._lib.mtg_cost_at_times_batch
        args = (self.handle, N, D, V - 1, r, B, _addr(vertex_values), None, _addr(times), C, _addr(scales),
                _addr(cost), None, nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC)
        handle = self.handle

        def call():
            rc = fn(*args)
            if rc:
                nat.check(rc, handle)
        return call

    def jacobian_call(self, N, r, vertex_values, times, scales, cost, jac, increment_time=0.0):
        """Zero-argument callable: one asynchronous device-pointer mtg_time_jacobian_batch launch on
        torch's current stream (the config-5 bench step: cost sweep + time Jacobian, matrix cores)."""
        import torch
        B, V, h, D = vertex_values.shape
        C = scales.shape[0]
        self.set_stream(torch.cuda.current_stream(vertex_values.device).cuda_stream)
        fn = self._lib.mtg_time_jacobian_batch
        args = (self.handle, N, D, V - 1, r, B, _addr(vertex_values), _addr(times), C, _addr(scales),
                float(increment_time), _addr(cost), _addr(jac), nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC)
        handle = self.handle

        def call():
            rc = fn(*args)
            if rc:
                nat.check(rc, handle)
        return call

    # ------------------------------------------------------------------ solve
    def solve_linear_batch(self, N, r, values, mask, times, coeffs=None, free=None, n_free=None,
                           cost=None, status=None, split=False, asynchronous=False, general=False, dl=False,
                           column=False):
        """Solve a batch; returns dict of outputs (allocates those not given).

        want-flags: pass arrays (or True to allocate) for free / n_free / cost / status."""
        dev = _is_torch(values) and values.is_cuda
        B, V, h, D = values.shape
        K = V - 1
        assert h == N // 2, "values must be [B][K+1][N/2][D]"
        assert tuple(mask.shape) == (B, V) and tuple(times.shape) == (B, K)
        out = {}

        def alloc(name, arr, shape, dtype):
            if arr is None or arr is False:
                return None
            if arr is True:
                if dev:
                    import torch
                    tdt = {np.float64: torch.float64, np.int32: torch.int32}[dtype]
                    arr = torch.empty(shape, dtype=tdt, device=values.device)
                else:
                    arr = np.empty(shape, dtype=dtype)
            out[name] = arr
            return arr

        coeffs = alloc("coeffs", True if coeffs is None else coeffs, (B, K, D, N), np.float64)
        free = alloc("free", free, (B, D, V * h), np.float64)
        n_free = alloc("n_free", n_free, (B,), np.int32)
        cost = alloc("cost", cost, (B,), np.float64)
        status = alloc("status", status, (B,), np.int32)
        flags = 0
        if dev:
            import torch
            flags |= nat.MTG_FLAG_DEVICE_PTRS
            self.set_stream(torch.cuda.current_stream(values.device).cuda_stream)
            if asynchronous:
                flags |= nat.MTG_FLAG_ASYNC
        else:
            values = np.ascontiguousarray(values, dtype=np.float64)
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            times = np.ascontiguousarray(times, dtype=np.float64)
            self.reset_stream()
        if split:
            flags |= nat.MTG_FLAG_SPLIT_KERNELS
        if general:
            flags |= nat.MTG_FLAG_GENERAL_KERNEL
        if dl:
            flags |= nat.MTG_FLAG_DL_KERNEL
        if column:
            flags |= nat.MTG_FLAG_COLUMN_KERNEL
        rc = self._lib.mtg_solve_linear_batch(self.handle, N, D, K, r, B, _addr(values), _addr(mask),
                                              _addr(times), _addr(coeffs), _addr(free), _addr(n_free),
                                              _addr(cost), _addr(status), flags)
        nat.check(rc, self.handle)
        return out

    def solve_linear_ragged_batch(self, N, r, values, mask, times, seg_count, coeffs=None, free=None, n_free=None,
                                  cost=None, status=None, split=False, asynchronous=False, general=False, dl=False,
                                  column=False):
        """Solve a batch whose trajectories have different segment counts (mtg_solve_linear_ragged_batch).

        The arrays are the CSR arrays of include/mtg.h (pack_ragged builds them): values [sum V][N/2][D],
        mask [sum V], times [sum K], numpy or torch-device; seg_count [B] is a host array (numpy or a
        list) either way.  Returns a dict of the outputs: coeffs [sum K][D][N], free (flat, D N/2 sum V
        doubles), n_free / cost / status [B]; split_ragged gives per-trajectory views.  The want-flags are
        those of solve_linear_batch; coeffs=False leaves the coefficients out."""
        dev = _is_torch(values) and values.is_cuda
        seg_count = np.ascontiguousarray(seg_count, dtype=np.int32)
        B = int(seg_count.shape[0])
        totS = int(seg_count.sum(dtype=np.int64))
        totV = totS + B
        h = N // 2
        assert values.ndim == 3 and values.shape[1] == h, "values must be [sum V][N/2][D]"
        D = int(values.shape[2])
        assert int(values.shape[0]) == totV and tuple(mask.shape) == (totV,) and tuple(times.shape) == (totS,)
        out = {}

        def alloc(name, arr, shape, dtype):
            if arr is None or arr is False:
                return None
            if arr is True:
                if dev:
                    import torch
                    tdt = {np.float64: torch.float64, np.int32: torch.int32}[dtype]
                    arr = torch.empty(shape, dtype=tdt, device=values.device)
                else:
                    arr = np.empty(shape, dtype=dtype)
            out[name] = arr
            return arr

        coeffs = alloc("coeffs", True if coeffs is None else coeffs, (totS, D, N), np.float64)
        free = alloc("free", free, (totV * h * D,), np.float64)
        n_free = alloc("n_free", n_free, (B,), np.int32)
        cost = alloc("cost", cost, (B,), np.float64)
        status = alloc("status", status, (B,), np.int32)
        flags = 0
        if dev:
            import torch
            flags |= nat.MTG_FLAG_DEVICE_PTRS
            self.set_stream(torch.cuda.current_stream(values.device).cuda_stream)
            if asynchronous:
                flags |= nat.MTG_FLAG_ASYNC
        else:
            values = np.ascontiguousarray(values, dtype=np.float64)
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            times = np.ascontiguousarray(times, dtype=np.float64)
            self.reset_stream()
        if split:
            flags |= nat.MTG_FLAG_SPLIT_KERNELS
        if general:
            flags |= nat.MTG_FLAG_GENERAL_KERNEL
        if dl:
            flags |= nat.MTG_FLAG_DL_KERNEL
        if column:
            flags |= nat.MTG_FLAG_COLUMN_KERNEL
        rc = self._lib.mtg_solve_linear_ragged_batch(self.handle, N, D, r, B, _addr(seg_count), _addr(values),
                                                     _addr(mask), _addr(times), _addr(coeffs), _addr(free),
                                                     _addr(n_free), _addr(cost), _addr(status), flags)
        nat.check(rc, self.handle)
        return out

    def time_sweep_batch(self, N, r, values, mask, times, scales, cost=None, status=None,
                         asynchronous=False, split=False, dl=False, column=False, general=False):
        dev = _is_torch(values) and values.is_cuda
        B, V, h, D = values.shape
        K = V - 1
        C = len(scales)
        if dev:
            import torch
            cost = cost if cost is not None else torch.empty((B, C), dtype=torch.float64, device=values.device)
            flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
            self.set_stream(torch.cuda.current_stream(values.device).cuda_stream)
        else:
            values = np.ascontiguousarray(values, dtype=np.float64)
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            times = np.ascontiguousarray(times, dtype=np.float64)
            scales = np.ascontiguousarray(scales, dtype=np.float64)
            cost = cost if cost is not None else np.empty((B, C))
            flags = 0
            self.reset_stream()
        if split:
            flags |= nat.MTG_FLAG_SPLIT_KERNELS
        if dl:
            flags |= nat.MTG_FLAG_DL_KERNEL
        if column:
            flags |= nat.MTG_FLAG_COLUMN_KERNEL
        if general:
            flags |= nat.MTG_FLAG_GENERAL_KERNEL
        rc = self._lib.mtg_time_sweep_batch(self.handle, N, D, K, r, B, _addr(values), _addr(mask),
                                            _addr(times), C, _addr(scales), _addr(cost), _addr(status), flags)
        nat.check(rc, self.handle)
        return cost

    def cost_at_times_batch(self, N, r, vertex_values, times, scales, mask=None, grad=False):
        """getCostAndGradientDerivative at candidate times (include/mtg.h mtg_cost_at_times_batch):
        cost [B][C] = sum_dims d^T R(T_c) d, and with grad=True (needs mask) grad [B][C][D][V*h] =
        2 (R(T_c) d)_free in the reference's free order.  scales [C][K] multiply times [B][K]."""
        vertex_values = np.ascontiguousarray(vertex_values, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64)
        scales = np.ascontiguousarray(scales, dtype=np.float64)
        B, V, h, D = vertex_values.shape
        K = V - 1
        C = scales.shape[0]
        assert scales.shape == (C, K) and times.shape == (B, K)
        cost = np.empty((B, C))
        g = np.zeros((B, C, D, V * h)) if grad else None
        m = np.ascontiguousarray(mask, dtype=np.uint8) if mask is not None else None
        self.reset_stream()
        nat.check(self._lib.mtg_cost_at_times_batch(self.handle, N, D, K, r, B, _addr(vertex_values), _addr(m),
                                                    _addr(times), C, _addr(scales), _addr(cost), _addr(g), 0),
                  self.handle)
        return (cost, g) if grad else cost

    def collision_cost_batch(self, N, vertex_values, times, grid, params, mask=None, grad=False, asynchronous=False):
        """getCostAndGradientCollision for a batch (include/mtg.h mtg_collision_cost_batch): vertex_values
        [B][V][h][3] (all derivatives), times [B][K], grid an SdfGrid, params a CollisionParams.  numpy
        arrays (staged, the grid included) or torch CUDA tensors (then grid.distance is one too, the
        launch goes to torch's current stream and asynchronous=True does not wait for it).  Returns
        dict(cost [B], collision [B] uint8, n_evaluated [B] int32, status [B] int32) and, with grad=True
        (needs mask), grad [B][3][V*h] packed as cost_at_times_batch's."""
        dev = _is_torch(vertex_values) and vertex_values.is_cuda
        B, V, h, D = vertex_values.shape
        K = V - 1
        assert h == N // 2 and tuple(times.shape) == (B, K)
        assert not grad or mask is not None, "grad needs mask"
        if dev:
            import torch
            assert _is_torch(grid.distance) and grid.distance.is_cuda, "device call: grid.distance must be a CUDA tensor"
            kw = dict(device=vertex_values.device)
            out = {"cost": torch.empty(B, dtype=torch.float64, **kw),
                   "collision": torch.empty(B, dtype=torch.uint8, **kw),
                   "n_evaluated": torch.empty(B, dtype=torch.int32, **kw),
                   "status": torch.empty(B, dtype=torch.int32, **kw)}
            if grad:
                out["grad"] = torch.empty((B, D, V * h), dtype=torch.float64, **kw)
            flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
            self.set_stream(torch.cuda.current_stream(vertex_values.device).cuda_stream)
        else:
            vertex_values = np.ascontiguousarray(vertex_values, dtype=np.float64)
            times = np.ascontiguousarray(times, dtype=np.float64)
            mask = np.ascontiguousarray(mask, dtype=np.uint8) if mask is not None else None
            out = {"cost": np.empty(B), "collision": np.empty(B, np.uint8), "n_evaluated": np.empty(B, np.int32),
                   "status": np.empty(B, np.int32)}
            if grad:
                out["grad"] = np.zeros((B, D, V * h))
            flags = 0
            self.reset_stream()
        g, keep = grid.native()
        nat.check(self._lib.mtg_collision_cost_batch(self.handle, N, D, K, B, _addr(vertex_values),
                                                     _addr(mask) if grad else None, _addr(times), ctypes.byref(g),
                                                     ctypes.byref(params.native()), _addr(out["cost"]),
                                                     _addr(out.get("grad")), _addr(out["collision"]),
                                                     _addr(out["n_evaluated"]), _addr(out["status"]), flags),
                  self.handle)
        del keep
        return out

    def collision_time_gradient_batch(self, N, vertex_values, times, grid, params, increment_time=0.1,
                                      asynchronous=False, diagnostics=True):
        """The collision part dJc_dt of getCostAndGradientTime for a batch (include/mtg.h
        mtg_collision_time_gradient_batch): the central difference of the collision cost in each segment
        time, walking the unperturbed polynomials to the perturbed end.  Arguments as
        collision_cost_batch (numpy arrays, or torch CUDA tensors with grid.distance one too).  Returns
        dict(grad_t [B][K], side_cost [B][K][2], side_evaluated [B][K][2] int32, segments_walked [B] int32,
        status [B] int32); diagnostics=False passes NULL for everything but grad_t and status (the others
        are then None; grad_t's bits do not change)."""
        dev = _is_torch(vertex_values) and vertex_values.is_cuda
        B, V, h, D = vertex_values.shape
        K = V - 1
        assert h == N // 2 and tuple(times.shape) == (B, K)
        shapes = (("grad_t", (B, K), "f8"), ("side_cost", (B, K, 2), "f8"), ("side_evaluated", (B, K, 2), "i4"),
                  ("segments_walked", (B,), "i4"), ("status", (B,), "i4"))
        if dev:
            import torch
            assert _is_torch(grid.distance) and grid.distance.is_cuda, "device call: grid.distance must be a CUDA tensor"
            out = {k: torch.empty(s, dtype=torch.float64 if t == "f8" else torch.int32, device=vertex_values.device)
                   for k, s, t in shapes}
            flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
            self.set_stream(torch.cuda.current_stream(vertex_values.device).cuda_stream)
        else:
            vertex_values = np.ascontiguousarray(vertex_values, dtype=np.float64)
            times = np.ascontiguousarray(times, dtype=np.float64)
            out = {k: np.empty(s, dtype=np.float64 if t == "f8" else np.int32) for k, s, t in shapes}
            flags = 0
            self.reset_stream()
        if not diagnostics:
            out["side_cost"] = out["side_evaluated"] = out["segments_walked"] = None
        g, keep = grid.native()
        nat.check(self._lib.mtg_collision_time_gradient_batch(
            self.handle, N, D, K, B, _addr(vertex_values), _addr(times), ctypes.byref(g), ctypes.byref(params.native()),
            float(increment_time), _addr(out["grad_t"]), _addr(out["side_cost"]), _addr(out["side_evaluated"]),
            _addr(out["segments_walked"]), _addr(out["status"]), flags), self.handle)
        del keep
        return out

    def time_gradient_batch(self, N, r, vertex_values, times, grid, params, weights=(0.1, 10.0, 1.0), increment_time=0.1):
        """The complete getCostAndGradientTime (nl_impl:2155-2243) for a batch, composed of
        time_jacobian_batch (dJd_dt: one candidate, scales of 1, the same increment_time) and
        collision_time_gradient_batch (dJc_dt).  weights = (w_d, w_c, w_t), the reference's defaults 0.1,
        10, 1.  The reference's w_sc dJsc_dt is 0 by its own code (updateSegmentTimes does not rebuild
        the segments its soft-constraint term reads, so it differences two equal numbers) and is left
        out.  numpy arrays.  Returns dict(J_t [B] = sum_i T_i, grad_t [B][K] = (w_d dJd_dt + w_c dJc_dt) +
        w_t, dJd_dt, dJc_dt, status [B])."""
        w_d, w_c, w_t = (float(w) for w in weights)
        times = np.ascontiguousarray(times, dtype=np.float64)
        K = times.shape[1]
        _, jd = self.time_jacobian_batch(N, r, vertex_values, times, np.ones((1, K)), increment_time=increment_time)
        c = self.collision_time_gradient_batch(N, vertex_values, times, grid, params, increment_time=increment_time,
                                               diagnostics=False)
        jd = jd[:, 0, :]
        return {"J_t": times.sum(1), "grad_t": (w_d * jd + w_c * c["grad_t"]) + w_t, "dJd_dt": jd, "dJc_dt": c["grad_t"],
                "status": c["status"]}

    def objective_batch(self, N, values, mask, x, params, times=None, grid=None, collision=None, soft=None, state=None,
                        grad=True, parts=False, asynchronous=False):
        """One evaluation of the reference's nonlinear objective per trajectory, in the optimiser's variables
        (include/mtg.h mtg_objective_batch): x [B][x_stride] holds (objective 2: the K segment times, then)
        D blocks of n_free[b] free derivatives; values / mask are the problem as solve_linear_batch reads
        it; params an ObjectiveParams; times [B][K] for objectives 0 and 1; grid / collision (SdfGrid,
        CollisionParams) for objectives 1 and 2; soft a SoftConstraintParams iff
        params.use_soft_constraints.  numpy arrays (staged once) or torch CUDA tensors (then grid.distance
        and state are tensors too, the launches go to torch's current stream and asynchronous=True does
        not wait for them).  state (optional, in/out): OBJECTIVE_STATE_DTYPE [B], or a torch uint8 tensor
        [B][48] holding the same records.  Returns dict(cost [B], grad [B][x_stride] or None,
        weighted_costs [B][4], collision [B] uint8, status [B] int32, state) and with parts=True the
        unweighted parts J_d, J_c, J_sc, J_t, dJd_dt, dJc_dt, grad_d, grad_c, grad_sc (None where the
        objective does not compute one)."""
        return _objective_call(self, N, values, mask, x, params, times, grid, collision, soft, state, grad, parts,
                               asynchronous, None)

    def objective_time_batch(self, N, values, mask, x, params, coeff_times=None, grid=None, collision=None,
                             constraints=None, state=None, parts=False, constraint_values=False, maxima=False,
                             free=False, coeffs=False, asynchronous=False):
        """One evaluation of objectiveFunctionTime (objective 3) or objectiveFunctionTimeAndConstraints
        (objective 4) per trajectory (include/mtg.h mtg_objective_time_batch): x [B][x_stride] holds the K
        segment times (objective 4: then D blocks of n_free[b] free derivatives); values / mask are the
        problem as solve_linear_batch reads it; params an ObjectiveTimeParams; coeff_times [B][K], grid
        and collision iff objective 3 with w_c > 0 (the collision walk's coefficients are formed at
        coeff_times: the reference's stale L_); constraints a SoftConstraintParams, needed with
        use_soft_constraints, constraint_values or maxima.  numpy arrays or torch CUDA tensors, state and
        asynchronous as in objective_batch.  Returns the keys of objective_batch (grad is None: these
        objectives have none; parts=True gives J_d (objective 4), J_c, J_sc, J_t) plus
        constraint_values [B][C] (maxima.value - limit: the hard inequality constraints' values), maxima
        (as soft_constraint_cost_batch returns them), free [B][D][V*h] and coeffs [B][K][D][N], each
        None unless requested."""
        return _objective_time_call(self, N, values, mask, x, params, coeff_times, grid, collision, constraints, state,
                                    parts, constraint_values, maxima, free, coeffs, asynchronous, None)

    def soft_constraint_cost_batch(self, N, vertex_values, times, params, mask=None, grad=False, asynchronous=False):
        """getCostAndGradientSoftConstraints for a batch (include/mtg.h mtg_soft_constraint_cost_batch):
        vertex_values [B][V][h][D] (all derivatives), times [B][K], params a SoftConstraintParams.  numpy
        arrays (staged) or torch CUDA tensors (the launch then goes to torch's current stream and
        asynchronous=True does not wait for it).  Returns dict(cost [B], grad, maxima [B][C], status [B]
        int32): grad is None unless grad=True (needs mask), then [B][D][V*h] packed as
        cost_at_times_batch's; maxima is a structured array (time, value, segment) for numpy input and
        for torch input a float64 tensor [B][C][3] holding the same 24-byte records
        (.cpu().numpy().view(EXTREMUM_DTYPE)[..., 0] decodes it)."""
        dev = _is_torch(vertex_values) and vertex_values.is_cuda
        B, V, h, D = vertex_values.shape
        K = V - 1
        assert h == N // 2 and tuple(times.shape) == (B, K)
        assert not grad or mask is not None, "grad needs mask"
        p = params.native()
        C = max(int(p.n_constraints), 1)
        if dev:
            import torch
            kw = dict(device=vertex_values.device)
            out = {"cost": torch.empty(B, dtype=torch.float64, **kw),
                   "grad": torch.empty((B, D, V * h), dtype=torch.float64, **kw) if grad else None,
                   "maxima": torch.zeros((B, C, 3), dtype=torch.float64, **kw),
                   "status": torch.empty(B, dtype=torch.int32, **kw)}
            flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
            self.set_stream(torch.cuda.current_stream(vertex_values.device).cuda_stream)
        else:
            vertex_values = np.ascontiguousarray(vertex_values, dtype=np.float64)
            times = np.ascontiguousarray(times, dtype=np.float64)
            mask = np.ascontiguousarray(mask, dtype=np.uint8) if mask is not None else None
            out = {"cost": np.empty(B), "grad": np.zeros((B, D, V * h)) if grad else None,
                   "maxima": np.zeros((B, C), dtype=EXTREMUM_DTYPE), "status": np.empty(B, np.int32)}
            flags = 0
            self.reset_stream()
        nat.check(self._lib.mtg_soft_constraint_cost_batch(self.handle, N, D, K, B, _addr(vertex_values),
                                                           _addr(mask) if grad else None, _addr(times),
                                                           ctypes.byref(p), _addr(out["cost"]), _addr(out["grad"]),
                                                           _addr(out["maxima"]), _addr(out["status"]), flags),
                  self.handle)
        return out

    def time_jacobian_batch(self, N, r, vertex_values, times, scales, increment_time=0.0, jacobian=True):
        """Cost sweep + segment-time Jacobian on the matrix cores (include/mtg.h mtg_time_jacobian_batch):
        cost [B][C] = sum_dims d^T R(T_c) d and jac [B][C][K] = dJ/dT_i at T_c (exact for
        increment_time == 0, the reference's central difference otherwise)."""
        vertex_values = np.ascontiguousarray(vertex_values, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64)
        scales = np.ascontiguousarray(scales, dtype=np.float64)
        B, V, h, D = vertex_values.shape
        K = V - 1
        C = scales.shape[0]
        assert scales.shape == (C, K) and times.shape == (B, K)
        cost = np.empty((B, C))
        jac = np.empty((B, C, K)) if jacobian else None
        self.reset_stream()
        nat.check(self._lib.mtg_time_jacobian_batch(self.handle, N, D, K, r, B, _addr(vertex_values), _addr(times),
                                                    C, _addr(scales), float(increment_time), _addr(cost),
                                                    _addr(jac), 0), self.handle)
        return (cost, jac) if jacobian else cost

    def coefficients_from_vertices_batch(self, N, vertex_values, times):
        """setFreeConstraints + updateSegmentsFromCompactConstraints (include/mtg.h
        mtg_coefficients_from_vertices_batch): [B][V][h][D] all vertex derivatives -> [B][K][D][N]."""
        vertex_values = np.ascontiguousarray(vertex_values, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64)
        B, V, h, D = vertex_values.shape
        K = V - 1
        assert h == N // 2 and times.shape == (B, K)
        out = np.empty((B, K, D, N))
        self.reset_stream()
        nat.check(self._lib.mtg_coefficients_from_vertices_batch(self.handle, N, D, K, B, _addr(vertex_values),
                                                                 _addr(times), _addr(out), 0), self.handle)
        return out

    def vertex_derivatives_batch(self, coeffs, times):
        """M^+ A p (include/mtg.h mtg_vertex_derivatives_batch): [B][K][D][N] -> [B][V][h][D]."""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64)
        B, K, D, N = coeffs.shape
        assert times.shape == (B, K)
        out = np.empty((B, K + 1, N // 2, D))
        self.reset_stream()
        nat.check(self._lib.mtg_vertex_derivatives_batch(self.handle, N, D, K, B, _addr(coeffs), _addr(times),
                                                         _addr(out), 0), self.handle)
        return out

    def vertex_derivatives_ragged_batch(self, coeffs, times, seg_count, asynchronous=False):
        """vertex_derivatives_batch for a batch of different segment counts
        (mtg_vertex_derivatives_ragged_batch): coeffs [sum K][D][N] and times [sum K] are the CSR arrays
        Context.solve_linear_ragged_batch returns and takes (numpy or torch-device), seg_count [B] a host
        array either way.  Returns vertex_values [sum K + B][N/2][D] (split_ragged kind "vertex_values");
        every trajectory's rows are the bytes vertex_derivatives_batch gives for it alone, and there is no
        limit on K."""
        coeffs, times = _csr(coeffs), _csr(times)
        seg_count, B, D, N = _ragged_coeff_shape(coeffs, times, seg_count)
        shape = (int(coeffs.shape[0]) + B, N // 2, D)
        coeffs, times, out, flags = self._ragged_map_arrays(coeffs, times, shape, asynchronous)
        nat.check(self._lib.mtg_vertex_derivatives_ragged_batch(self.handle, N, D, B, _addr(seg_count), _addr(coeffs),
                                                                _addr(times), _addr(out), flags), self.handle)
        return out

    def coefficients_from_vertices_ragged_batch(self, N, vertex_values, times, seg_count, asynchronous=False):
        """coefficients_from_vertices_batch for a batch of different segment counts
        (mtg_coefficients_from_vertices_ragged_batch): vertex_values [sum K + B][N/2][D] (all derivatives)
        and times [sum K], numpy or torch-device; seg_count [B] a host array.  Returns coeffs [sum K][D][N];
        every trajectory's block is the bytes coefficients_from_vertices_batch gives for it alone."""
        vertex_values, times = _csr(vertex_values), _csr(times)
        seg_count, B, D = _ragged_vertex_shape(N, vertex_values, times, seg_count)
        shape = (int(times.shape[0]), D, N)
        vertex_values, times, out, flags = self._ragged_map_arrays(vertex_values, times, shape, asynchronous)
        nat.check(self._lib.mtg_coefficients_from_vertices_ragged_batch(self.handle, N, D, B, _addr(seg_count),
                                                                        _addr(vertex_values), _addr(times), _addr(out),
                                                                        flags), self.handle)
        return out

    def _ragged_map_arrays(self, a, times, out_shape, asynchronous):
        """The contiguous inputs, the output array and the flags of a ragged vertex-map call."""
        if _is_torch(a) and a.is_cuda:
            import torch
            out = torch.empty(out_shape, dtype=torch.float64, device=a.device)
            self.set_stream(torch.cuda.current_stream(a.device).cuda_stream)
            return a.contiguous(), times.contiguous(), out, nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
        self.reset_stream()
        return (np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(times, dtype=np.float64),
                np.empty(out_shape), 0)

    def collision_cost_ragged_batch(self, N, vertex_values, times, seg_count, grid, params, mask=None, grad=False,
                                    asynchronous=False):
        """collision_cost_batch for a batch of different segment counts (mtg_collision_cost_ragged_batch):
        vertex_values [sum K + B][N/2][3] (all derivatives), mask [sum K + B] and times [sum K] are CSR arrays
        (numpy, or torch-device with a torch grid.distance), seg_count [B] a host array either way.  Returns
        dict(cost, collision, n_evaluated, status), each [B], and with grad=True (needs mask) grad, flat
        3 N/2 (sum K + B) doubles in the layout of solve_linear_ragged_batch's free (split_ragged kind
        "grad").  Every trajectory's outputs are the bytes collision_cost_batch gives for it alone."""
        vertex_values, times = _csr(vertex_values), _csr(times)
        dev = _is_torch(vertex_values) and vertex_values.is_cuda
        seg_count, B, D = _ragged_vertex_shape(N, vertex_values, times, seg_count)
        totV, h = int(vertex_values.shape[0]), N // 2
        assert not grad or mask is not None, "grad needs mask"
        assert mask is None or tuple(mask.shape) == (totV,), "mask must be [sum K + B]"
        if dev:
            import torch
            assert _is_torch(grid.distance) and grid.distance.is_cuda, "device call: grid.distance must be a CUDA tensor"
            kw = dict(device=vertex_values.device)
            vertex_values, times = vertex_values.contiguous(), times.contiguous()
            mask = mask.contiguous() if mask is not None else None
            out = {"cost": torch.empty(B, dtype=torch.float64, **kw),
                   "collision": torch.empty(B, dtype=torch.uint8, **kw),
                   "n_evaluated": torch.empty(B, dtype=torch.int32, **kw),
                   "status": torch.empty(B, dtype=torch.int32, **kw)}
            if grad:
                out["grad"] = torch.empty((totV * h * D,), dtype=torch.float64, **kw)
            flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
            self.set_stream(torch.cuda.current_stream(vertex_values.device).cuda_stream)
        else:
            vertex_values = np.ascontiguousarray(vertex_values, dtype=np.float64)
            times = np.ascontiguousarray(times, dtype=np.float64)
            mask = np.ascontiguousarray(mask, dtype=np.uint8) if mask is not None else None
            out = {"cost": np.empty(B), "collision": np.empty(B, np.uint8), "n_evaluated": np.empty(B, np.int32),
                   "status": np.empty(B, np.int32)}
            if grad:
                out["grad"] = np.zeros((totV * h * D,))
            flags = 0
            self.reset_stream()
        g, keep = grid.native()
        nat.check(self._lib.mtg_collision_cost_ragged_batch(self.handle, N, D, B, _addr(seg_count), _addr(vertex_values),
                                                            _addr(mask) if grad else None, _addr(times), ctypes.byref(g),
                                                            ctypes.byref(params.native()), _addr(out["cost"]),
                                                            _addr(out.get("grad")), _addr(out["collision"]),
                                                            _addr(out["n_evaluated"]), _addr(out["status"]), flags),
                  self.handle)
        del keep
        return out

    def set_free_constraints_batch(self, N, values, mask, times, free):
        """PolynomialOptimization::setFreeConstraints (polynomial_optimization_linear.h:185-186) for a
        batch: the fixed values stay, the free derivatives come from `free` [B][D][V*h] (reference
        order); returns the recomputed coefficients [B][K][D][N] (lin_impl:253-273)."""
        return self.coefficients_from_vertices_batch(N, full_vertex_values(values, mask, free, N), times)

    def initial_solution_without_position_constraints(self, N, r, values, mask, times):
        """PolynomialOptimizationNonLinear::computeInitialSolutionWithoutPositionConstraints
        (polynomial_optimization_nonlinear_impl.h:116-187) for a batch: solve, drop every position
        constraint except at the first and last vertex, and start the new free derivatives from the
        solved trajectory (M^+ A p).  Returns dict(mask, values, free [B][D][V*h], n_free, coeffs):
        the new problem (mask, values) and its free-constraint vector.  Setting that vector back
        (set_free_constraints_batch) reproduces the solved trajectory up to rounding; re-solving the new
        problem does not, because the freed interior positions move.  Both vertex maps stage whole
        trajectories in LDS (include/mtg.h: at D = 3, K <= 66 for N = 10 and K <= 55 for N = 12, else
        MTG_ERR_TOO_LARGE), so the long chains (K = 100) are outside this function."""
        values = np.ascontiguousarray(values, dtype=np.float64)
        B, V, h, D = values.shape
        sol = self.solve_linear_batch(N, r, values, mask, times)
        allv = self.vertex_derivatives_batch(sol["coeffs"], times)
        new_mask = np.array(mask, dtype=np.uint8, copy=True)
        new_mask[:, 1:V - 1] &= np.uint8(0xFE)  # vertices_[k].removeConstraint(POSITION), 0 < k < V-1
        fixed = ((new_mask[:, :, None] >> np.arange(h)[None, None, :]) & 1).astype(bool)  # [B][V][h]
        free = np.zeros((B, D, V * h))
        n_free = np.zeros(B, dtype=np.int32)
        for b in range(B):
            slots = np.flatnonzero(~fixed[b].reshape(-1))  # reference (vertex, derivative) order
            n_free[b] = len(slots)
            free[b, :, :len(slots)] = allv[b].reshape(-1, D)[slots].T
        return {"mask": new_mask, "values": values, "free": free, "n_free": n_free, "coeffs": sol["coeffs"]}

    def min_max_magnitude_batch(self, coeffs, times, derivative, dimensions=None):
        """Trajectory::computeMinMaxMagnitude (src/trajectory.cpp:181-218) for a batch (include/mtg.h
        mtg_min_max_magnitude_batch).  Returns (minimum, maximum), structured arrays [B] with fields
        time (segment-local), value, segment."""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64)
        B, K, D, N = coeffs.shape
        mask = 0 if dimensions is None else int(sum(1 << int(d) for d in dimensions))
        mn = np.zeros(B, dtype=EXTREMUM_DTYPE)
        mx = np.zeros(B, dtype=EXTREMUM_DTYPE)
        self.reset_stream()
        nat.check(self._lib.mtg_min_max_magnitude_batch(self.handle, N, D, K, B, _addr(coeffs), _addr(times),
                                                        int(derivative), mask, _addr(mn), _addr(mx), 0),
                  self.handle)
        return mn, mx

    # ------------------------------------------------------- evaluateRange
    def evaluate_range_batch(self, coeffs, times, t_start, t_end, dt, derivative=0, want_times=True):
        """Host-array convenience wrapper: returns (samples [S][D], sample_times [S], counts [B], offsets [B])."""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64)
        B, K, D, N = coeffs.shape
        counts = np.zeros(B, dtype=np.int64)
        self.reset_stream()
        nat.check(self._lib.mtg_evaluate_range_batch(self.handle, N, D, K, B, None, _addr(times), t_start, t_end,
                                                     dt, derivative, _addr(counts), None, None, None, 0),
                  self.handle)
        offsets = np.zeros(B, dtype=np.int64)
        if B > 1:
            offsets[1:] = np.cumsum(counts)[:-1]
        total = int(counts.sum())
        out = np.zeros((max(total, 1), D))
        st = np.zeros(max(total, 1)) if want_times else None
        nat.check(self._lib.mtg_evaluate_range_batch(self.handle, N, D, K, B, _addr(coeffs), _addr(times), t_start,
                                                     t_end, dt, derivative, _addr(counts), _addr(offsets),
                                                     _addr(out), _addr(st), 0), self.handle)
        return out[:total], (st[:total] if want_times else None), counts, offsets

    def evaluate_range_batch_full(self, coeffs, times, t_start, t_end, dt, derivative=0, want_times=True,
                                  capacity=None, asynchronous=False):
        """Trajectory::evaluateRange for the batch in one call (mtg_evaluate_range_batch_full): counts,
        offsets and samples computed on the device without a host round trip.  numpy arrays or torch
        CUDA tensors (then every output is a device tensor on torch's current stream).  capacity: rows
        of the sample buffer (default: evaluate_range_capacity, a safe bound); the call is retried
        once with the exact total if it was short.  Returns (samples [S][D], sample_times [S] or None,
        counts [B], offsets [B]); with asynchronous=True (device tensors only) the full-capacity
        buffers and the device total are returned instead of the trimmed views: (samples, times,
        counts, offsets, total)."""
        dev = _is_torch(coeffs) and coeffs.is_cuda
        B, K, D, N = coeffs.shape
        if capacity is None:
            capacity = evaluate_range_capacity(times, t_start, t_end, dt)
        for attempt in range(2):
            if dev:
                import torch
                kw = dict(device=coeffs.device)
                counts = torch.empty(B, dtype=torch.int64, **kw)
                offsets = torch.empty(B, dtype=torch.int64, **kw)
                total = torch.zeros(1, dtype=torch.int64, **kw)
                out = torch.empty((max(capacity, 1), D), dtype=torch.float64, **kw)
                st = torch.empty(max(capacity, 1), dtype=torch.float64, **kw) if want_times else None
                flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
                self.set_stream(torch.cuda.current_stream(coeffs.device).cuda_stream)
            else:
                coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
                times = np.ascontiguousarray(times, dtype=np.float64)
                counts = np.empty(B, dtype=np.int64)
                offsets = np.empty(B, dtype=np.int64)
                total = np.zeros(1, dtype=np.int64)
                out = np.empty((max(capacity, 1), D))
                st = np.empty(max(capacity, 1)) if want_times else None
                flags = 0
                self.reset_stream()
            rc = self._lib.mtg_evaluate_range_batch_full(self.handle, N, D, K, B, _addr(coeffs), _addr(times),
                                                         float(t_start), float(t_end), float(dt), int(derivative),
                                                         _addr(counts), _addr(offsets), _addr(total), _addr(out),
                                                         _addr(st), int(capacity), flags)
            if dev and asynchronous:
                nat.check(rc, self.handle)
                return out, st, counts, offsets, total
            if rc == nat.MTG_ERR_TOO_LARGE and attempt == 0:
                capacity = int(total[0])
                continue
            nat.check(rc, self.handle)
            break
        n = int(total[0])
        return out[:n], (st[:n] if want_times else None), counts, offsets


    # --------------------------------------------------------- evaluate
    def evaluate_at_batch(self, coeffs, times, t_query, derivative_begin=0, n_derivatives=1, want_in_range=True,
                          asynchronous=False):
        """Trajectory::evaluate of every trajectory at caller-given times (include/mtg.h
        mtg_evaluate_at_batch): coeffs [B][K][D][N], times [B][K]; t_query [M] (one row of times shared by
        the batch) or [B][M], also as a view whose rows are contiguous and at least M elements apart.
        numpy arrays or torch CUDA tensors (then the launch goes to torch's current stream and
        asynchronous=True does not wait for it).  Returns (out [B][M][n_derivatives][D] with the orders
        derivative_begin .. derivative_begin + n_derivatives - 1, in_range [B][M] uint8 or None,
        status [B] int32)."""
        dev = _is_torch(coeffs) and coeffs.is_cuda
        B, K, D, N = coeffs.shape
        assert tuple(times.shape) == (B, K)
        if dev:
            import torch
            kw = dict(device=coeffs.device)
            coeffs, times = coeffs.contiguous(), times.contiguous()
            t_query, t_stride, M = _query_rows(t_query, B, lambda a: a.stride(), lambda a: a.contiguous())
            out = torch.empty((B, M, n_derivatives, D), dtype=torch.float64, **kw)
            in_range = torch.empty((B, M), dtype=torch.uint8, **kw) if want_in_range else None
            status = torch.empty(B, dtype=torch.int32, **kw)
            flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
            self.set_stream(torch.cuda.current_stream(coeffs.device).cuda_stream)
        else:
            coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
            times = np.ascontiguousarray(times, dtype=np.float64)
            t_query, t_stride, M = _query_rows_numpy(t_query, B)
            out = np.empty((B, M, n_derivatives, D))
            in_range = np.empty((B, M), np.uint8) if want_in_range else None
            status = np.empty(B, np.int32)
            flags = 0
            self.reset_stream()
        nat.check(self._lib.mtg_evaluate_at_batch(self.handle, N, D, K, B, _addr(coeffs), _addr(times), _addr(t_query),
                                                  t_stride, M, int(derivative_begin), int(n_derivatives), _addr(out),
                                                  _addr(in_range), _addr(status), flags), self.handle)
        return out, in_range, status

    # --------------------------------------------- ragged K, after the solve
    def evaluate_at_ragged_batch(self, coeffs, times, seg_count, t_query, derivative_begin=0, n_derivatives=1,
                                 want_in_range=True, asynchronous=False):
        """evaluate_at_batch for a batch of different segment counts (mtg_evaluate_at_ragged_batch): coeffs
        [sum K][D][N] and times [sum K] are the CSR arrays Context.solve_linear_ragged_batch returns and takes
        (numpy or torch-device), seg_count [B] a host array either way; t_query, the other arguments and the
        result are those of evaluate_at_batch.  Every trajectory's rows are the bytes evaluate_at_batch gives
        for it alone.  coeffs and times may also be lists of per-trajectory blocks (split_ragged): joined first."""
        coeffs, times = _csr(coeffs), _csr(times)
        dev = _is_torch(coeffs) and coeffs.is_cuda
        seg_count, B, D, N = _ragged_coeff_shape(coeffs, times, seg_count)
        if dev:
            import torch
            kw = dict(device=coeffs.device)
            coeffs, times = coeffs.contiguous(), times.contiguous()
            t_query, t_stride, M = _query_rows(t_query, B, lambda a: a.stride(), lambda a: a.contiguous())
            out = torch.empty((B, M, n_derivatives, D), dtype=torch.float64, **kw)
            in_range = torch.empty((B, M), dtype=torch.uint8, **kw) if want_in_range else None
            status = torch.empty(B, dtype=torch.int32, **kw)
            flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
            self.set_stream(torch.cuda.current_stream(coeffs.device).cuda_stream)
        else:
            coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
            times = np.ascontiguousarray(times, dtype=np.float64)
            t_query, t_stride, M = _query_rows_numpy(t_query, B)
            out = np.empty((B, M, n_derivatives, D))
            in_range = np.empty((B, M), np.uint8) if want_in_range else None
            status = np.empty(B, np.int32)
            flags = 0
            self.reset_stream()
        nat.check(self._lib.mtg_evaluate_at_ragged_batch(self.handle, N, D, B, _addr(seg_count), _addr(coeffs),
                                                         _addr(times), _addr(t_query), t_stride, M,
                                                         int(derivative_begin), int(n_derivatives), _addr(out),
                                                         _addr(in_range), _addr(status), flags), self.handle)
        return out, in_range, status

    def evaluate_range_ragged_batch(self, coeffs, times, seg_count, t_start, t_end, dt, derivative=0, want_times=True):
        """evaluate_range_batch for a batch of different segment counts (mtg_evaluate_range_ragged_batch, the
        two-call form on host arrays): coeffs [sum K][D][N], times [sum K], seg_count [B].  Returns (samples
        [S][D], sample_times [S] or None, counts [B], offsets [B]); every trajectory's samples are the bytes
        evaluate_range_batch gives for it alone.  coeffs and times may also be lists of per-trajectory blocks
        (split_ragged)."""
        coeffs = np.ascontiguousarray(_csr(coeffs), dtype=np.float64)
        times = np.ascontiguousarray(_csr(times), dtype=np.float64)
        seg_count, B, D, N = _ragged_coeff_shape(coeffs, times, seg_count)
        counts = np.zeros(B, dtype=np.int64)
        self.reset_stream()
        nat.check(self._lib.mtg_evaluate_range_ragged_batch(self.handle, N, D, B, _addr(seg_count), None, _addr(times),
                                                            float(t_start), float(t_end), float(dt), int(derivative),
                                                            _addr(counts), None, None, None, 0), self.handle)
        offsets = np.zeros(B, dtype=np.int64)
        if B > 1:
            offsets[1:] = np.cumsum(counts)[:-1]
        total = int(counts.sum())
        out = np.zeros((max(total, 1), D))
        st = np.zeros(max(total, 1)) if want_times else None
        nat.check(self._lib.mtg_evaluate_range_ragged_batch(self.handle, N, D, B, _addr(seg_count), _addr(coeffs),
                                                            _addr(times), float(t_start), float(t_end), float(dt),
                                                            int(derivative), _addr(counts), _addr(offsets), _addr(out),
                                                            _addr(st), 0), self.handle)
        return out[:total], (st[:total] if want_times else None), counts, offsets

    def evaluate_range_ragged_batch_full(self, coeffs, times, seg_count, t_start, t_end, dt, derivative=0,
                                         want_times=True, capacity=None, asynchronous=False):
        """evaluate_range_batch_full for a batch of different segment counts
        (mtg_evaluate_range_ragged_batch_full): the CSR arrays coeffs [sum K][D][N] and times [sum K] as
        Context.solve_linear_ragged_batch returns them (numpy or torch-device), seg_count [B] a host array
        either way.  capacity, the retry, asynchronous and the result are those of evaluate_range_batch_full."""
        coeffs, times = _csr(coeffs), _csr(times)
        dev = _is_torch(coeffs) and coeffs.is_cuda
        seg_count, B, D, N = _ragged_coeff_shape(coeffs, times, seg_count)
        if capacity is None:
            capacity = evaluate_range_capacity(times, t_start, t_end, dt, seg_count=seg_count)
        for attempt in range(2):
            if dev:
                import torch
                kw = dict(device=coeffs.device)
                coeffs, times = coeffs.contiguous(), times.contiguous()
                counts = torch.empty(B, dtype=torch.int64, **kw)
                offsets = torch.empty(B, dtype=torch.int64, **kw)
                total = torch.zeros(1, dtype=torch.int64, **kw)
                out = torch.empty((max(capacity, 1), D), dtype=torch.float64, **kw)
                st = torch.empty(max(capacity, 1), dtype=torch.float64, **kw) if want_times else None
                flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
                self.set_stream(torch.cuda.current_stream(coeffs.device).cuda_stream)
            else:
                coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
                times = np.ascontiguousarray(times, dtype=np.float64)
                counts = np.empty(B, dtype=np.int64)
                offsets = np.empty(B, dtype=np.int64)
                total = np.zeros(1, dtype=np.int64)
                out = np.empty((max(capacity, 1), D))
                st = np.empty(max(capacity, 1)) if want_times else None
                flags = 0
                self.reset_stream()
            rc = self._lib.mtg_evaluate_range_ragged_batch_full(self.handle, N, D, B, _addr(seg_count), _addr(coeffs),
                                                                _addr(times), float(t_start), float(t_end), float(dt),
                                                                int(derivative), _addr(counts), _addr(offsets),
                                                                _addr(total), _addr(out), _addr(st), int(capacity),
                                                                flags)
            if dev and asynchronous:
                nat.check(rc, self.handle)
                return out, st, counts, offsets, total
            if rc == nat.MTG_ERR_TOO_LARGE and attempt == 0:
                capacity = int(total[0])
                continue
            nat.check(rc, self.handle)
            break
        n = int(total[0])
        return out[:n], (st[:n] if want_times else None), counts, offsets

    def min_max_magnitude_ragged_batch(self, coeffs, times, seg_count, derivative, dimensions=None, minimum=True,
                                       maximum=True, asynchronous=False):
        """min_max_magnitude_batch for a batch of different segment counts
        (mtg_min_max_magnitude_ragged_batch): coeffs [sum K][D][N], times [sum K] (numpy or torch-device) and
        the host array seg_count [B].  Returns (minimum, maximum), each a structured array [B]
        (EXTREMUM_DTYPE; for device arrays a torch uint8 tensor [B][24] on the device, see extrema_from_bytes)
        or None where minimum=False / maximum=False.  Every entry is the bytes min_max_magnitude_batch gives
        for that trajectory alone.  coeffs and times may also be lists of per-trajectory blocks (split_ragged)."""
        coeffs, times = _csr(coeffs), _csr(times)
        dev = _is_torch(coeffs) and coeffs.is_cuda
        seg_count, B, D, N = _ragged_coeff_shape(coeffs, times, seg_count)
        mask = 0 if dimensions is None else int(sum(1 << int(d) for d in dimensions))
        if dev:
            import torch
            coeffs, times = coeffs.contiguous(), times.contiguous()
            mn, mx = (torch.zeros((B, EXTREMUM_DTYPE.itemsize), dtype=torch.uint8, device=coeffs.device) if want else None
                      for want in (minimum, maximum))
            flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
            self.set_stream(torch.cuda.current_stream(coeffs.device).cuda_stream)
        else:
            coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
            times = np.ascontiguousarray(times, dtype=np.float64)
            mn, mx = (np.zeros(B, dtype=EXTREMUM_DTYPE) if want else None for want in (minimum, maximum))
            flags = 0
            self.reset_stream()
        nat.check(self._lib.mtg_min_max_magnitude_ragged_batch(self.handle, N, D, B, _addr(seg_count), _addr(coeffs),
                                                               _addr(times), int(derivative), mask, _addr(mn),
                                                               _addr(mx), flags), self.handle)
        return mn, mx

    # ------------------------------------------------ per-segment extrema
    def segment_min_max_magnitude_batch(self, coeffs, times, derivative, dimensions=None, windows=None, **outputs):
        """Minimum and maximum magnitude of every segment on its window, with the candidate list
        (include/mtg.h mtg_segment_min_max_magnitude_batch: Segment::computeMinMaxMagnitudeCandidates +
        selectMinMaxMagnitudeFromCandidates).  coeffs [S][D][N] and times [S] have no trajectory structure: a
        uniform batch reshaped to [B K] and the CSR arrays of a ragged batch are both valid.  windows [S][2]
        (t_start, t_end; None: [0, times[s]], and times may be None when windows is given).  numpy arrays or
        torch CUDA tensors (then every output is a device tensor on torch's current stream; the extrema are
        uint8 [S][24], see extrema_from_bytes).  outputs: minimum=True, maximum=True, candidate_capacity=0
        (> 0: candidate_times [S][capacity]), candidate_count=True, status=True, asynchronous=False.  Returns a
        dict of the requested outputs."""
        return _segment_extrema(self, False, coeffs, times, derivative, dimensions, windows, **outputs)

    def segment_min_max_axis_batch(self, coeffs, times, derivative, windows=None, **outputs):
        """Signed minimum and maximum of every (segment, dimension) on its window (mtg_segment_min_max_axis_batch:
        Polynomial::computeMinMax): arguments and outputs as segment_min_max_magnitude_batch, with minimum /
        maximum [S][D], candidate_times [S][D][capacity] and candidate_count [S][D]."""
        return _segment_extrema(self, True, coeffs, times, derivative, None, windows, **outputs)


def _segment_extrema(ctx, axis, coeffs, times, derivative, dimensions, windows, minimum=True, maximum=True,
                     candidate_capacity=0, candidate_count=True, status=True, asynchronous=False, threads=1):
    """The four per-segment entries; ctx None: the host path."""
    dev = _is_torch(coeffs) and coeffs.is_cuda
    S, D, N = (int(x) for x in coeffs.shape)
    assert times is not None or windows is not None, "times or windows is required"
    assert times is None or tuple(times.shape) == (S,), "times must be [S]"
    assert windows is None or tuple(windows.shape) == (S, 2), "windows must be [S][2]"
    mask = 0 if dimensions is None else int(sum(1 << int(d) for d in dimensions))
    cap = int(candidate_capacity)
    item = (S, D) if axis else (S,)
    if dev:
        import torch
        assert ctx is not None, "the host path takes numpy arrays"
        kw = dict(device=coeffs.device)
        coeffs = coeffs.contiguous()
        times = None if times is None else times.contiguous()
        windows = None if windows is None else windows.contiguous()
        mn, mx = (torch.zeros(item + (EXTREMUM_DTYPE.itemsize,), dtype=torch.uint8, **kw) if want else None
                  for want in (minimum, maximum))
        cand = torch.empty(item + (cap,), dtype=torch.float64, **kw) if cap > 0 else None
        cnt = torch.empty(item, dtype=torch.int32, **kw) if candidate_count else None
        stat = torch.empty(S, dtype=torch.int32, **kw) if status else None
        flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
        ctx.set_stream(torch.cuda.current_stream(coeffs.device).cuda_stream)
    else:
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        times = None if times is None else np.ascontiguousarray(times, dtype=np.float64)
        windows = None if windows is None else np.ascontiguousarray(windows, dtype=np.float64)
        mn, mx = (np.zeros(item, dtype=EXTREMUM_DTYPE) if want else None for want in (minimum, maximum))
        cand = np.empty(item + (cap,)) if cap > 0 else None
        cnt = np.empty(item, np.int32) if candidate_count else None
        stat = np.empty(S, np.int32) if status else None
        flags = 0
        if ctx is not None:
            ctx.reset_stream()
    head = (N, D, S, _addr(coeffs), _addr(times), _addr(windows), int(derivative))
    tail = (_addr(mn), _addr(mx), _addr(cand), _addr(cnt), cap, _addr(stat))
    if ctx is None:
        lib = nat.load()
        if axis:
            nat.check(lib.mtg_host_segment_min_max_axis_batch(*head, *tail, threads))
        else:
            nat.check(lib.mtg_host_segment_min_max_magnitude_batch(*head, mask, *tail, threads))
    elif axis:
        nat.check(ctx._lib.mtg_segment_min_max_axis_batch(ctx.handle, *head, *tail, flags), ctx.handle)
    else:
        nat.check(ctx._lib.mtg_segment_min_max_magnitude_batch(ctx.handle, *head, mask, *tail, flags), ctx.handle)
    return {"minimum": mn, "maximum": mx, "candidate_times": cand, "candidate_count": cnt, "status": stat}


def host_segment_min_max_magnitude_batch(coeffs, times, derivative, dimensions=None, windows=None, **outputs):
    """Context.segment_min_max_magnitude_batch on the library's host path
    (mtg_host_segment_min_max_magnitude_batch): no GPU, numpy arrays; outputs also takes threads=1."""
    return _segment_extrema(None, False, coeffs, times, derivative, dimensions, windows, **outputs)


def host_segment_min_max_axis_batch(coeffs, times, derivative, windows=None, **outputs):
    """Context.segment_min_max_axis_batch on the library's host path (mtg_host_segment_min_max_axis_batch)."""
    return _segment_extrema(None, True, coeffs, times, derivative, None, windows, **outputs)


def extrema_from_bytes(t):
    """The structured array [B] (EXTREMUM_DTYPE) of a device result of min_max_magnitude_ragged_batch (a torch
    uint8 tensor [B][24]); waits for the tensor's stream."""
    return np.ascontiguousarray(t.cpu().numpy()).view(EXTREMUM_DTYPE).reshape(-1)


def join_ragged(per_trajectory):
    """One CSR array of per-trajectory blocks (what split_ragged yields: coeffs [K_b][D][N] or times [K_b]),
    numpy or torch; a copy."""
    per_trajectory = list(per_trajectory)
    if per_trajectory and _is_torch(per_trajectory[0]):
        import torch
        return torch.cat(per_trajectory)
    return np.concatenate([np.asarray(x, dtype=np.float64) for x in per_trajectory])


def _csr(x):
    """A CSR array as it is; a list of per-trajectory blocks (split_ragged) joined."""
    return join_ragged(x) if isinstance(x, (list, tuple)) else x


def _ragged_coeff_shape(coeffs, times, seg_count):
    """(seg_count as int32, B, D, N) of the CSR arrays coeffs [sum K][D][N], times [sum K]."""
    seg_count = np.ascontiguousarray(seg_count, dtype=np.int32).reshape(-1)
    totS = int(seg_count.sum(dtype=np.int64))
    assert coeffs.ndim == 3 and int(coeffs.shape[0]) == totS, "coeffs must be [sum K][D][N]"
    assert tuple(times.shape) == (totS,), "times must be [sum K]"
    return seg_count, int(seg_count.shape[0]), int(coeffs.shape[1]), int(coeffs.shape[2])


def _ragged_vertex_shape(N, vertex_values, times, seg_count):
    """(seg_count as int32, B, D) of the CSR arrays vertex_values [sum K + B][N/2][D], times [sum K]."""
    seg_count = np.ascontiguousarray(seg_count, dtype=np.int32).reshape(-1)
    B, totS = int(seg_count.shape[0]), int(seg_count.sum(dtype=np.int64))
    assert vertex_values.ndim == 3 and int(vertex_values.shape[0]) == totS + B and int(vertex_values.shape[1]) == N // 2, \
        "vertex_values must be [sum K + B][N/2][D]"
    assert tuple(times.shape) == (totS,), "times must be [sum K]"
    return seg_count, B, int(vertex_values.shape[2])


def _query_rows(t_query, B, strides, contiguous):
    """(array, t_stride, M) of evaluate_at's query times: [M] is shared (stride 0); [B][M] keeps its row
    stride when its rows are contiguous and at least M elements apart, else it is made contiguous."""
    if t_query.ndim == 1:
        return contiguous(t_query), 0, int(t_query.shape[0])
    assert t_query.ndim == 2 and t_query.shape[0] == B, "t_query must be [M] or [B][M]"
    M = int(t_query.shape[1])
    s = strides(t_query)
    if M > 0 and B > 0 and not (s[1] == 1 and (s[0] >= M or B == 1)):
        t_query = contiguous(t_query)
        s = (M, 1)
    return t_query, (max(int(s[0]), M) if M > 0 else 0), M


def _query_rows_numpy(t_query, B):
    t_query = np.asarray(t_query, dtype=np.float64)
    return _query_rows(t_query, B, lambda a: tuple(x // a.itemsize for x in a.strides), np.ascontiguousarray)


def host_evaluate_at_batch(coeffs, times, t_query, derivative_begin=0, n_derivatives=1, want_in_range=True, threads=0):
    """Context.evaluate_at_batch on the library's host path (mtg_host_evaluate_at_batch): no GPU; the same
    bits as the kernels.  numpy arrays; threads <= 0: mtg_host_default_threads()."""
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    B, K, D, N = coeffs.shape
    assert tuple(times.shape) == (B, K)
    t_query, t_stride, M = _query_rows_numpy(t_query, B)
    out = np.empty((B, M, n_derivatives, D))
    in_range = np.empty((B, M), np.uint8) if want_in_range else None
    status = np.empty(B, np.int32)
    nat.check(nat.load().mtg_host_evaluate_at_batch(N, D, K, B, _addr(coeffs), _addr(times), _addr(t_query), t_stride,
                                                    M, int(derivative_begin), int(n_derivatives), _addr(out),
                                                    _addr(in_range), _addr(status), int(threads)))
    return out, in_range, status


def evaluate_range_capacity(times, t_start, t_end, dt, seg_count=None):
    """A safe sample capacity for evaluateRange over a batch (mtg_evaluate_range_batch_full): per
    trajectory the clock samples while the accumulated time (>= 0) is below t_end and the sample is
    inside the trajectory, so at most min(t_end, sum T) / dt + 2 samples; 1e-9 relative slack for the
    rounding of the accumulated clock.  times [B][K], or with seg_count [B] the CSR array [sum K]
    (mtg_evaluate_range_ragged_batch_full): the same bound per trajectory, summed."""
    if _is_torch(times):
        times = times.detach().cpu().numpy()
    times = np.asarray(times, dtype=np.float64)
    if seg_count is None:
        duration = times.sum(axis=1)
    else:
        seg_count = np.asarray(seg_count, dtype=np.int64).reshape(-1)
        assert (seg_count >= 1).all() and times.shape == (int(seg_count.sum()),), "times must be [sum K], K_b >= 1"
        duration = np.add.reduceat(times, np.cumsum(seg_count) - seg_count) if len(seg_count) else np.zeros(0)
    span = np.minimum(duration, float(t_end))
    n = np.floor(np.maximum(span, 0.0) / float(dt) * (1.0 + 1e-9)) + 3
    return int(n.sum())


def full_vertex_values(values, mask, free, N):
    """All derivatives of every vertex [B][V][h][D]: the fixed values where the mask says fixed,
    the solved free values (free_out [B][D][V*h], reference order) elsewhere."""
    values = np.asarray(values, dtype=np.float64)
    B, V, h, D = values.shape
    fixed = ((np.asarray(mask)[:, :, None] >> np.arange(h)[None, None, :]) & 1).astype(bool)  # [B][V][h]
    out = np.where(fixed[..., None], values, 0.0)
    for b in range(B):
        slots = np.flatnonzero(~fixed[b].reshape(-1))  # (v, k) of free derivatives, reference order
        for d in range(D):
            out[b].reshape(-1, D)[slots, d] = free[b, d, :len(slots)]
    return out


_default_ctx = {}


def default_context(device=0):
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = _default_ctx[device] = Context(device)
    return ctx


def solve_linear_batch(N, r, values, mask, times, device=0, **kw):
    return default_context(device).solve_linear_batch(N, r, values, mask, times, **kw)


def collision_cost_batch(N, vertex_values, times, grid, params, device=0, **kw):
    return default_context(device).collision_cost_batch(N, vertex_values, times, grid, params, **kw)


def soft_constraint_cost_batch(N, vertex_values, times, params, device=0, **kw):
    return default_context(device).soft_constraint_cost_batch(N, vertex_values, times, params, **kw)


def collision_time_gradient_batch(N, vertex_values, times, grid, params, device=0, **kw):
    return default_context(device).collision_time_gradient_batch(N, vertex_values, times, grid, params, **kw)


def time_gradient_batch(N, r, vertex_values, times, grid, params, device=0, **kw):
    return default_context(device).time_gradient_batch(N, r, vertex_values, times, grid, params, **kw)


def shard_range(batch, n_shards, shard):
    """[begin, end) of contiguous shard `shard` of `n_shards` (mtg_shard_range)."""
    b, e = ctypes.c_int64(0), ctypes.c_int64(0)
    nat.check(nat.load().mtg_shard_range(batch, n_shards, shard, ctypes.byref(b), ctypes.byref(e)))
    return b.value, e.value


def solve_linear_batch_multi(contexts, N, r, values, mask, times, free=False, n_free=False, cost=False,
                             status=False):
    """One batch over several contexts (normally one per device) in one call
    (mtg_solve_linear_batch_multi): contiguous shards, one host thread per context, host arrays in and
    out; bit-identical to one Context.solve_linear_batch over the whole batch."""
    lib = nat.load()
    values = np.ascontiguousarray(values, dtype=np.float64)
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    times = np.ascontiguousarray(times, dtype=np.float64)
    B, V, h, D = values.shape
    K = V - 1
    assert h == N // 2 and mask.shape == (B, V) and times.shape == (B, K)
    out = {"coeffs": np.empty((B, K, D, N))}
    if free:
        out["free"] = np.zeros((B, D, V * h))
    if n_free:
        out["n_free"] = np.empty((B,), np.int32)
    if cost:
        out["cost"] = np.empty((B,))
    if status:
        out["status"] = np.empty((B,), np.int32)
    handles = (ctypes.c_void_p * len(contexts))(*[c.handle for c in contexts])
    rc = lib.mtg_solve_linear_batch_multi(ctypes.cast(handles, ctypes.c_void_p), len(contexts), N, D, K, r, B,
                                          _addr(values), _addr(mask), _addr(times), _addr(out["coeffs"]),
                                          _addr(out.get("free")), _addr(out.get("n_free")), _addr(out.get("cost")),
                                          _addr(out.get("status")), 0)
    nat.check(rc, contexts[0].handle)
    return out


class SdfGrid:
    """struct mtg_sdf_grid (include/mtg.h): a dense signed distance field, distance [nx][ny][nz] float32
    (numpy, or a torch CUDA tensor for device calls), origin = the low corner of cell (0, 0, 0),
    resolution = the cell edge, oob_distance = the value outside the grid."""

    def __init__(self, distance, origin, resolution, oob_distance=0.0):
        if not _is_torch(distance):
            distance = np.ascontiguousarray(distance, dtype=np.float32)
        else:
            import torch
            assert distance.dtype == torch.float32 and distance.is_contiguous()
        assert len(distance.shape) == 3
        self.distance = distance
        self.origin = tuple(float(x) for x in origin)
        self.resolution = float(resolution)
        self.oob_distance = float(oob_distance)

    def native(self):
        """(the ctypes struct, the array it points into: keep it alive for the call)"""
        nx, ny, nz = (int(n) for n in self.distance.shape)
        g = nat.SdfGrid(_addr(self.distance), nx, ny, nz, (ctypes.c_double * 3)(*self.origin), self.resolution,
                        self.oob_distance)
        return g, self.distance


class CollisionParams:
    """struct mtg_collision_params (include/mtg.h), the reference's optimization_parameters_ fields of the
    collision term: dt = coll_check_time_increment; map_resolution is the arc-length gate, the bounds
    margin and the finite-difference increment."""

    def __init__(self, dt, map_resolution, epsilon, robot_radius, coll_pot_multiplier=1.0, min_bound=(0.0, 0.0, 0.0),
                 max_bound=(0.0, 0.0, 0.0), use_continuous_distance=False):
        self.dt = float(dt)
        self.map_resolution = float(map_resolution)
        self.epsilon = float(epsilon)
        self.robot_radius = float(robot_radius)
        self.coll_pot_multiplier = float(coll_pot_multiplier)
        self.min_bound = tuple(float(x) for x in min_bound)
        self.max_bound = tuple(float(x) for x in max_bound)
        self.use_continuous_distance = bool(use_continuous_distance)

    def native(self):
        return nat.CollisionParams(self.dt, self.map_resolution, self.epsilon, self.robot_radius,
                                   self.coll_pot_multiplier, (ctypes.c_double * 3)(*self.min_bound),
                                   (ctypes.c_double * 3)(*self.max_bound), int(self.use_continuous_distance), 0)


def host_collision_cost_batch(N, vertex_values, times, grid, params, mask=None, grad=False, threads=1):
    """The library's host path of Context.collision_cost_batch (mtg_host_collision_cost_batch): the
    reference's loop in scalar C++, no GPU.  Same arguments (numpy arrays) and outputs."""
    lib = nat.load()
    vertex_values = np.ascontiguousarray(vertex_values, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    B, V, h, D = vertex_values.shape
    K = V - 1
    assert h == N // 2 and times.shape == (B, K)
    assert not grad or mask is not None, "grad needs mask"
    mask = np.ascontiguousarray(mask, dtype=np.uint8) if mask is not None else None
    out = {"cost": np.empty(B), "collision": np.empty(B, np.uint8), "n_evaluated": np.empty(B, np.int32),
           "status": np.empty(B, np.int32)}
    if grad:
        out["grad"] = np.zeros((B, D, V * h))
    g, keep = grid.native()
    nat.check(lib.mtg_host_collision_cost_batch(N, D, K, B, _addr(vertex_values), _addr(mask) if grad else None,
                                                _addr(times), ctypes.byref(g), ctypes.byref(params.native()),
                                                _addr(out["cost"]), _addr(out.get("grad")), _addr(out["collision"]),
                                                _addr(out["n_evaluated"]), _addr(out["status"]), threads))
    del keep
    return out


def host_collision_time_gradient_batch(N, vertex_values, times, grid, params, increment_time=0.1, threads=1):
    """The library's host path of Context.collision_time_gradient_batch
    (mtg_host_collision_time_gradient_batch): the reference written literally, 2K complete walks per
    trajectory, no GPU.  Same arguments (numpy arrays) and outputs, without segments_walked."""
    lib = nat.load()
    vertex_values = np.ascontiguousarray(vertex_values, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    B, V, h, D = vertex_values.shape
    K = V - 1
    assert h == N // 2 and times.shape == (B, K)
    out = {"grad_t": np.empty((B, K)), "side_cost": np.empty((B, K, 2)), "side_evaluated": np.empty((B, K, 2), np.int32),
           "status": np.empty(B, np.int32)}
    g, keep = grid.native()
    nat.check(lib.mtg_host_collision_time_gradient_batch(N, D, K, B, _addr(vertex_values), _addr(times), ctypes.byref(g),
                                                         ctypes.byref(params.native()), float(increment_time),
                                                         _addr(out["grad_t"]), _addr(out["side_cost"]),
                                                         _addr(out["side_evaluated"]), _addr(out["status"]), threads))
    del keep
    return out


class SoftConstraintParams:
    """struct mtg_soft_constraint_params (include/mtg.h): the magnitude limits of
    addMaximumMagnitudeConstraint as (derivative, limit) pairs, with the reference's
    soft_constraint_weight, maximum cost and finite-difference increment (its map_resolution)."""

    def __init__(self, constraints, weight=100.0, maximum_cost=1e12, increment=0.05):
        self.constraints = [(int(k), float(v)) for k, v in constraints]
        self.weight = float(weight)
        self.maximum_cost = float(maximum_cost)
        self.increment = float(increment)

    def native(self):
        n = len(self.constraints)
        c = self.constraints[:8] + [(0, 0.0)] * (8 - min(n, 8))
        return nat.SoftConstraintParams(n, (ctypes.c_int32 * 8)(*[k for k, _ in c]),
                                        (ctypes.c_double * 8)(*[v for _, v in c]), self.weight, self.maximum_cost,
                                        self.increment)


def host_soft_constraint_cost_batch(N, vertex_values, times, params, mask=None, grad=False, threads=1):
    """The library's host path of Context.soft_constraint_cost_batch (mtg_host_soft_constraint_cost_batch):
    the reference's loop written literally (every perturbation re-forms and searches the whole
    trajectory), no GPU.  Same arguments (numpy arrays) and outputs."""
    lib = nat.load()
    vertex_values = np.ascontiguousarray(vertex_values, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    B, V, h, D = vertex_values.shape
    K = V - 1
    assert h == N // 2 and times.shape == (B, K)
    assert not grad or mask is not None, "grad needs mask"
    mask = np.ascontiguousarray(mask, dtype=np.uint8) if mask is not None else None
    p = params.native()
    C = max(int(p.n_constraints), 1)
    out = {"cost": np.empty(B), "grad": np.zeros((B, D, V * h)) if grad else None,
           "maxima": np.zeros((B, C), dtype=EXTREMUM_DTYPE), "status": np.empty(B, np.int32)}
    nat.check(lib.mtg_host_soft_constraint_cost_batch(N, D, K, B, _addr(vertex_values), _addr(mask) if grad else None,
                                                      _addr(times), ctypes.byref(p), _addr(out["cost"]),
                                                      _addr(out["grad"]), _addr(out["maxima"]), _addr(out["status"]),
                                                      threads))
    return out


# struct mtg_objective_state (include/mtg.h); all-zero = a fresh optimisation
OBJECTIVE_STATE_DTYPE = np.dtype([("total_cost_iter0", "<f8"), ("cost_trajectory", "<f8"), ("cost_collision", "<f8"),
                                  ("cost_time", "<f8"), ("cost_soft_constraints", "<f8"), ("n_iterations", "<i4"),
                                  ("iter0_done", "<i4")])

OBJECTIVE_PARTS = ("J_d", "J_c", "J_sc", "J_t", "dJd_dt", "dJc_dt", "grad_d", "grad_c", "grad_sc")


class ObjectiveParams:
    """struct mtg_objective_params (include/mtg.h): which of the reference's objective functions
    (0 free constraints, 1 + collision, 2 + collision + time), the weights w_d, w_c, w_t, w_sc (reference
    defaults 0.1, 10, 1, 1), increment_time, and the "raise the cost while in collision" switches."""

    def __init__(self, objective, derivative_to_optimize, w_d=0.1, w_c=10.0, w_t=1.0, w_sc=1.0, increment_time=0.1,
                 use_soft_constraints=True, is_collision_safe=False, is_coll_raise_first_iter=True, add_coll_raise=0.0,
                 reserved=0):
        self.objective = int(objective)
        self.derivative_to_optimize = int(derivative_to_optimize)
        self.w_d, self.w_c, self.w_t, self.w_sc = float(w_d), float(w_c), float(w_t), float(w_sc)
        self.increment_time = float(increment_time)
        self.use_soft_constraints = bool(use_soft_constraints)
        self.is_collision_safe = bool(is_collision_safe)
        self.is_coll_raise_first_iter = bool(is_coll_raise_first_iter)
        self.add_coll_raise = float(add_coll_raise)
        self.reserved = int(reserved)

    def native(self):
        return nat.ObjectiveParams(self.objective, self.derivative_to_optimize, self.w_d, self.w_c, self.w_t, self.w_sc,
                                   self.increment_time, int(self.use_soft_constraints), int(self.is_collision_safe),
                                   int(self.is_coll_raise_first_iter), self.reserved, self.add_coll_raise)


def number_of_free_constraints(mask, N):
    """n_free [B]: the derivatives below N/2 that mask [B][V] does not fix (bit 7 and bits >= N/2 ignored)."""
    h = N // 2
    m = np.asarray(mask).astype(np.uint32)
    return (h - ((m[:, :, None] >> np.arange(h)[None, None, :]) & 1).sum(axis=2)).sum(axis=1).astype(np.int32)


def pack_optimization_variables(times, free, n_free, x_stride=None):
    """x [B][x_stride] in the layout of objective_batch: times [B][K] (or None: objectives 0 and 1), then
    for each of the D dimensions the first n_free[b] entries of free [B][D][*].  x_stride defaults to
    the longest row; the padding is 0."""
    free = np.asarray(free, dtype=np.float64)
    B, D = free.shape[0], free.shape[1]
    n_free = np.asarray(n_free)
    K = 0 if times is None else np.asarray(times).shape[1]
    longest = K + D * int(n_free.max()) if B else K
    stride = longest if x_stride is None else int(x_stride)
    assert stride >= longest, "x_stride is shorter than the longest row"
    x = np.zeros((B, stride))
    for b in range(B):
        nf = int(n_free[b])
        if K:
            x[b, :K] = np.asarray(times)[b]
        for d in range(D):
            x[b, K + d * nf:K + (d + 1) * nf] = free[b, d, :nf]
    return x


def unpack_optimization_variables(x, n_free, D, n_times=0, width=None):
    """The inverse of pack_optimization_variables: (times [B][n_times] or None, free [B][D][width]) with
    the entries past n_free[b] zero; width defaults to the largest n_free."""
    x = np.asarray(x, dtype=np.float64)
    n_free = np.asarray(n_free)
    B = x.shape[0]
    width = int(n_free.max()) if width is None and B else int(width or 0)
    free = np.zeros((B, D, width))
    for b in range(B):
        nf = int(n_free[b])
        for d in range(D):
            free[b, d, :nf] = x[b, n_times + d * nf:n_times + (d + 1) * nf]
    return (x[:, :n_times].copy() if n_times else None), free


def _objective_call(ctx, N, values, mask, x, params, times, grid, collision, soft, state, grad, parts, asynchronous,
                    threads):
    """Shared body of Context.objective_batch (ctx given) and host_objective_batch (ctx None)."""
    lib = nat.load()
    dev = ctx is not None and _is_torch(x) and x.is_cuda
    B, V, h, D = values.shape
    K = V - 1
    assert h == N // 2 and tuple(mask.shape) == (B, V) and x.shape[0] == B and len(x.shape) == 2
    stride = int(x.shape[1])
    p = params.native()
    with_coll, with_time, with_soft = p.objective >= 1, p.objective == 2, bool(p.use_soft_constraints)
    shapes = {"J_d": (B,), "J_c": (B,), "J_sc": (B,), "J_t": (B,), "dJd_dt": (B, K), "dJc_dt": (B, K),
              "grad_d": (B, D, V * h), "grad_c": (B, D, V * h), "grad_sc": (B, D, V * h)}
    have = {"J_d": True, "J_c": with_coll, "J_sc": with_soft, "J_t": True, "dJd_dt": grad and with_time,
            "dJc_dt": grad and with_time, "grad_d": grad, "grad_c": grad and with_coll,
            "grad_sc": grad and with_coll and with_soft}
    if dev:
        import torch
        kw = dict(device=x.device)
        assert grid is None or (_is_torch(grid.distance) and grid.distance.is_cuda), \
            "device call: grid.distance must be a CUDA tensor"
        assert x.is_contiguous() and values.is_contiguous() and mask.is_contiguous()

        def new(shape, dtype="f8"):
            return torch.zeros(shape, dtype={"f8": torch.float64, "u1": torch.uint8, "i4": torch.int32}[dtype], **kw)
        flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
        ctx.set_stream(torch.cuda.current_stream(x.device).cuda_stream)
    else:
        values = np.ascontiguousarray(values, dtype=np.float64)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        x = np.ascontiguousarray(x, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64) if times is not None else None
        if state is not None:
            assert state.dtype == OBJECTIVE_STATE_DTYPE and state.flags.c_contiguous and state.shape == (B,)

        def new(shape, dtype="f8"):
            return np.zeros(shape, dtype={"f8": np.float64, "u1": np.uint8, "i4": np.int32}[dtype])
        flags = 0
        if ctx is not None:
            ctx.reset_stream()
    assert times is None or tuple(times.shape) == (B, K)
    out = {"cost": new((B,)), "grad": new((B, stride)) if grad else None, "weighted_costs": new((B, 4)),
           "collision": new((B,), "u1"), "status": new((B,), "i4"), "state": state}
    for k in OBJECTIVE_PARTS:
        out[k] = new(shapes[k]) if parts and have[k] else None
    pp = nat.ObjectiveParts(*[_addr(out[k]) for k in OBJECTIVE_PARTS])
    g, keep = grid.native() if grid is not None else (None, None)
    cp = collision.native() if collision is not None else None
    sp = soft.native() if soft is not None else None
    tail = (_addr(x), stride, ctypes.byref(p), ctypes.byref(g) if g is not None else None,
            ctypes.byref(cp) if cp is not None else None, ctypes.byref(sp) if sp is not None else None,
            _addr(out["cost"]), _addr(out["grad"]), _addr(out["weighted_costs"]), _addr(out["collision"]), _addr(state),
            ctypes.byref(pp) if parts else None, _addr(out["status"]))
    if ctx is not None:
        nat.check(lib.mtg_objective_batch(ctx.handle, N, D, K, B, _addr(values), _addr(mask), _addr(times), *tail,
                                          flags), ctx.handle)
    else:
        nat.check(lib.mtg_host_objective_batch(N, D, K, B, _addr(values), _addr(mask), _addr(times), *tail, threads))
    del keep
    return out


def host_objective_batch(N, values, mask, x, params, times=None, grid=None, collision=None, soft=None, state=None,
                         grad=True, parts=False, threads=1):
    """The library's host path of Context.objective_batch (mtg_host_objective_batch), no GPU: same
    arguments (numpy arrays) and outputs."""
    return _objective_call(None, N, values, mask, x, params, times, grid, collision, soft, state, grad, parts, False,
                           threads)


def host_objective_bounds_batch(N, D, K, mask, x, derivative_to_optimize, with_times, solve_with_position_constraint,
                                constraints=None, min_bound=None, max_bound=None, initial_stepsize_rel=0.1):
    """Bounds and initial step of the optimiser's variables (mtg_host_objective_bounds_batch: the reference's
    setFreeEndpointDerivativeHardConstraints and the time bounds / initial step of its optimize set-up,
    restated literally).  mask [B][V], x [B][x_stride] in objective_batch's layout (with the K times first
    when with_times), constraints a SoftConstraintParams (its (derivative, limit) pairs) or None,
    min_bound / max_bound [D] (needed without the position constraint).  Returns (lower, upper,
    initial_step), each [B][x_stride]; raises MTGError(MTG_ERR_INVALID_ARGUMENT) where the reference's
    index runs past the end."""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    x = np.ascontiguousarray(x, dtype=np.float64)
    B, stride = x.shape
    assert mask.shape == (B, K + 1)
    lo, up, step = np.zeros((B, stride)), np.zeros((B, stride)), np.zeros((B, stride))
    mn = np.ascontiguousarray(min_bound, dtype=np.float64) if min_bound is not None else None
    mx = np.ascontiguousarray(max_bound, dtype=np.float64) if max_bound is not None else None
    cp = constraints.native() if constraints is not None else None
    nat.check(nat.load().mtg_host_objective_bounds_batch(
        N, D, K, B, _addr(mask), int(bool(with_times)), _addr(x), stride, int(derivative_to_optimize),
        int(bool(solve_with_position_constraint)), ctypes.byref(cp) if cp is not None else None, _addr(mn), _addr(mx),
        float(initial_stepsize_rel), _addr(lo), _addr(up), _addr(step)))
    return lo, up, step


class ObjectiveTimeParams:
    """struct mtg_objective_time_params (include/mtg.h): objective 3 (objectiveFunctionTime) or 4
    (objectiveFunctionTimeAndConstraints, the reference's default), time_penalty (reference default 500),
    w_c (objective 3 only: the collision term exists iff w_c > 0) and use_soft_constraints."""

    def __init__(self, objective, derivative_to_optimize, time_penalty=500.0, w_c=0.0, use_soft_constraints=True,
                 reserved=0):
        self.objective = int(objective)
        self.derivative_to_optimize = int(derivative_to_optimize)
        self.time_penalty = float(time_penalty)
        self.w_c = float(w_c)
        self.use_soft_constraints = bool(use_soft_constraints)
        self.reserved = int(reserved)

    def native(self):
        return nat.ObjectiveTimeParams(self.objective, self.derivative_to_optimize, self.time_penalty, self.w_c,
                                       int(self.use_soft_constraints), self.reserved)


OBJECTIVE_TIME_PARTS = ("J_d", "J_c", "J_sc", "J_t")


def _objective_time_call(ctx, N, values, mask, x, params, coeff_times, grid, collision, constraints, state, parts,
                         constraint_values, maxima, free, coeffs, asynchronous, threads):
    """Shared body of Context.objective_time_batch (ctx given) and host_objective_time_batch (ctx None)."""
    lib = nat.load()
    dev = ctx is not None and _is_torch(x) and x.is_cuda
    B, V, h, D = values.shape
    K = V - 1
    assert h == N // 2 and tuple(mask.shape) == (B, V) and x.shape[0] == B and len(x.shape) == 2
    assert coeff_times is None or tuple(coeff_times.shape) == (B, K)
    stride = int(x.shape[1])
    p = params.native()
    sp = constraints.native() if constraints is not None else None
    C = max(int(sp.n_constraints), 1) if sp is not None else 1
    assert sp is not None or not (constraint_values or maxima), "constraint_values / maxima need constraints"
    have = {"J_d": p.objective == nat.MTG_OBJECTIVE_TIME_AND_CONSTRAINTS,
            "J_c": p.objective == nat.MTG_OBJECTIVE_TIME and p.w_c > 0.0,
            "J_sc": bool(p.use_soft_constraints) or constraint_values or maxima, "J_t": True}
    if dev:
        import torch
        kw = dict(device=x.device)
        assert grid is None or (_is_torch(grid.distance) and grid.distance.is_cuda), \
            "device call: grid.distance must be a CUDA tensor"
        assert x.is_contiguous() and values.is_contiguous() and mask.is_contiguous()
        assert coeff_times is None or coeff_times.is_contiguous()

        def new(shape, dtype="f8"):
            return torch.zeros(shape, dtype={"f8": torch.float64, "u1": torch.uint8, "i4": torch.int32}[dtype], **kw)
        out_maxima = new((B, C, 3)) if maxima else None
        flags = nat.MTG_FLAG_DEVICE_PTRS | (nat.MTG_FLAG_ASYNC if asynchronous else 0)
        ctx.set_stream(torch.cuda.current_stream(x.device).cuda_stream)
    else:
        values = np.ascontiguousarray(values, dtype=np.float64)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        x = np.ascontiguousarray(x, dtype=np.float64)
        coeff_times = np.ascontiguousarray(coeff_times, dtype=np.float64) if coeff_times is not None else None
        if state is not None:
            assert state.dtype == OBJECTIVE_STATE_DTYPE and state.flags.c_contiguous and state.shape == (B,)

        def new(shape, dtype="f8"):
            return np.zeros(shape, dtype={"f8": np.float64, "u1": np.uint8, "i4": np.int32}[dtype])
        out_maxima = np.zeros((B, C), dtype=EXTREMUM_DTYPE) if maxima else None
        flags = 0
        if ctx is not None:
            ctx.reset_stream()
    out = {"cost": new((B,)), "grad": None, "weighted_costs": new((B, 4)), "collision": new((B,), "u1"),
           "status": new((B,), "i4"), "state": state,
           "constraint_values": new((B, C)) if constraint_values else None, "maxima": out_maxima,
           "free": new((B, D, V * h)) if free else None, "coeffs": new((B, K, D, N)) if coeffs else None}
    for k in OBJECTIVE_PARTS:
        out[k] = new((B,)) if parts and have.get(k) else None
    pp = nat.ObjectiveParts(*[_addr(out[k]) for k in OBJECTIVE_PARTS])
    g, keep = grid.native() if grid is not None else (None, None)
    cp = collision.native() if collision is not None else None
    tail = (_addr(values), _addr(mask), _addr(x), stride, ctypes.byref(p), _addr(coeff_times),
            ctypes.byref(g) if g is not None else None, ctypes.byref(cp) if cp is not None else None,
            ctypes.byref(sp) if sp is not None else None, _addr(out["cost"]), _addr(out["weighted_costs"]),
            _addr(out["collision"]), _addr(out["constraint_values"]), _addr(out["maxima"]), _addr(out["free"]),
            _addr(out["coeffs"]), _addr(state), ctypes.byref(pp) if parts else None, _addr(out["status"]))
    if ctx is not None:
        nat.check(lib.mtg_objective_time_batch(ctx.handle, N, D, K, B, *tail, flags), ctx.handle)
    else:
        nat.check(lib.mtg_host_objective_time_batch(N, D, K, B, *tail, threads))
    del keep
    return out


def host_objective_time_batch(N, values, mask, x, params, coeff_times=None, grid=None, collision=None,
                              constraints=None, state=None, parts=False, constraint_values=False, maxima=False,
                              free=False, coeffs=False, threads=1):
    """The library's host path of Context.objective_time_batch (mtg_host_objective_time_batch), no GPU: same
    arguments (numpy arrays) and outputs."""
    return _objective_time_call(None, N, values, mask, x, params, coeff_times, grid, collision, constraints, state,
                                parts, constraint_values, maxima, free, coeffs, False, threads)


def host_objective_time_bounds_batch(N, D, K, mask, x, objective, initial_stepsize_rel=0.1):
    """Bounds and initial step of the two set-ups (mtg_host_objective_time_bounds_batch, restated literally):
    objective 3: step = rel * t, lower 0.1, upper 2 t; objective 4: step = rel * |x|, bounds -+ 2 |x|, then
    lower 0.1 for the K times.  mask [B][V], x [B][x_stride] in objective_time_batch's layout.  Returns
    (lower, upper, initial_step), each [B][x_stride] with +0.0 past a row's length."""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    x = np.ascontiguousarray(x, dtype=np.float64)
    B, stride = x.shape
    assert mask.shape == (B, K + 1)
    lo, up, step = np.zeros((B, stride)), np.zeros((B, stride)), np.zeros((B, stride))
    nat.check(nat.load().mtg_host_objective_time_bounds_batch(N, D, K, B, _addr(mask), int(objective), _addr(x), stride,
                                                              float(initial_stepsize_rel), _addr(lo), _addr(up),
                                                              _addr(step)))
    return lo, up, step


def host_min_max_magnitude_batch(coeffs, times, derivative, dimensions=None, threads=1):
    """The library's host path of Context.min_max_magnitude_batch (mtg_host_min_max_magnitude_batch):
    Trajectory::computeMinMaxMagnitude on the CPU, as the reference computes it (src/trajectory.cpp:181-218)."""
    lib = nat.load()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    B, K, D, N = coeffs.shape
    mask = 0 if dimensions is None else int(sum(1 << int(d) for d in dimensions))
    mn = np.zeros(B, dtype=EXTREMUM_DTYPE)
    mx = np.zeros(B, dtype=EXTREMUM_DTYPE)
    nat.check(lib.mtg_host_min_max_magnitude_batch(N, D, K, B, _addr(coeffs), _addr(times), int(derivative), mask,
                                                   _addr(mn), _addr(mx), threads))
    return mn, mx


def host_solve_linear_batch(N, r, values, mask, times, free=False, n_free=False, cost=False, status=False,
                            threads=1):
    """The library's host (CPU) solve path (mtg_host_solve_linear_batch): same algorithm and outputs as
    Context.solve_linear_batch, no GPU.  The drop-in PolynomialOptimization<N>::solveLinear uses it for
    single problems (BASELINE config 1)."""
    lib = nat.load()
    values = np.ascontiguousarray(values, dtype=np.float64)
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    times = np.ascontiguousarray(times, dtype=np.float64)
    B, V, h, D = values.shape
    K = V - 1
    assert h == N // 2, "values must be [B][K+1][N/2][D]"
    assert mask.shape == (B, V) and times.shape == (B, K)
    out = {"coeffs": np.empty((B, K, D, N))}
    if free:
        out["free"] = np.empty((B, D, V * h))
    if n_free:
        out["n_free"] = np.empty((B,), np.int32)
    if cost:
        out["cost"] = np.empty((B,))
    if status:
        out["status"] = np.empty((B,), np.int32)
    nat.check(lib.mtg_host_solve_linear_batch(N, D, K, r, B, _addr(values), _addr(mask), _addr(times),
                                              _addr(out["coeffs"]), _addr(out.get("free")),
                                              _addr(out.get("n_free")), _addr(out.get("cost")),
                                              _addr(out.get("status")), threads))
    return out


# --------------------------------------------------------------------- ragged
def ragged_offsets(seg_count):
    """(vo, so) of the CSR layout (include/mtg.h, mtg_solve_linear_ragged_batch): int64 arrays of B + 1
    entries, vo[b] = sum_{j<b} (K_j + 1) and so[b] = sum_{j<b} K_j; the last entries are the totals."""
    k = np.asarray(seg_count, dtype=np.int64).reshape(-1)
    so = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    return so + np.arange(len(k) + 1, dtype=np.int64), so


def pack_ragged(problems):
    """CSR arrays of a list of problems, each (values [V][N/2][D], mask [V], times [K]) with V = K + 1:
    returns (values [sum V][N/2][D], mask [sum V], times [sum K], seg_count [B] int32)."""
    problems = list(problems)
    for v, m, t in problems:
        assert v.ndim == 3 and m.shape == (v.shape[0],) and t.shape == (v.shape[0] - 1,) and len(t) >= 1
    seg_count = np.array([len(t) for _, _, t in problems], dtype=np.int32)
    if not problems:
        return np.zeros((0, 0, 0)), np.zeros((0,), np.uint8), np.zeros((0,)), seg_count
    values = np.ascontiguousarray(np.concatenate([v for v, _, _ in problems]), dtype=np.float64)
    mask = np.ascontiguousarray(np.concatenate([m for _, m, _ in problems]), dtype=np.uint8)
    times = np.ascontiguousarray(np.concatenate([t for _, _, t in problems]), dtype=np.float64)
    return values, mask, times, seg_count


_RAGGED_KINDS = {"values": "vertex", "mask": "vertex", "times": "segment", "coeffs": "segment", "free": "free",
                 "n_free": "trajectory", "cost": "trajectory", "status": "trajectory",
                 # the ragged vertex maps and collision cost: all vertex derivatives, the gradient block (free's
                 # layout), and the collision entry's per-trajectory outputs
                 "vertex_values": "vertex", "grad": "free", "collision": "trajectory", "n_evaluated": "trajectory"}


def split_ragged(array, seg_count, kind, D=None):
    """Per-trajectory views (no copies) of one CSR array of a ragged batch, numpy or torch.  kind names
    the array: "values" -> [V_b][N/2][D], "mask" -> [V_b], "times" -> [K_b], "coeffs" -> [K_b][D][N],
    "free" -> [D][V_b N/2] (needs D), "n_free" / "cost" / "status" -> the entry of b; "vertex_values" as
    "values", "grad" (collision_cost_ragged_batch) as "free", "collision" / "n_evaluated" as "cost"."""
    what = _RAGGED_KINDS[kind]
    vo, so = ragged_offsets(seg_count)
    B = len(vo) - 1
    if what == "trajectory":
        return [array[b] for b in range(B)]
    if what == "free":
        assert D is not None, "split_ragged(..., '%s') needs D" % kind
        flat = array.reshape(-1)
        hD = int(flat.shape[0]) // max(int(vo[-1]), 1)
        return [flat[hD * int(vo[b]):hD * int(vo[b + 1])].reshape(D, -1) for b in range(B)]
    off = vo if what == "vertex" else so
    return [array[int(off[b]):int(off[b + 1])] for b in range(B)]


def solve_ragged_plan(N, D, r, seg_count, split=False, general=False, dl=False, column=False):
    """The plan mtg_solve_linear_ragged_batch makes for these segment counts (mtg_solve_ragged_plan; no
    device work): a dict with n_groups (distinct K), n_in_place (trajectories of groups that are one run of
    the batch, solved on slices of the caller's arrays; == B for a batch sorted by K) and total_segments."""
    lib = nat.load()
    addr, B = None, 0
    if seg_count is not None:
        seg_count = np.ascontiguousarray(seg_count, dtype=np.int32)
        addr, B = _addr(seg_count), int(seg_count.shape[0])
    flags = ((nat.MTG_FLAG_SPLIT_KERNELS if split else 0) | (nat.MTG_FLAG_GENERAL_KERNEL if general else 0) |
             (nat.MTG_FLAG_DL_KERNEL if dl else 0) | (nat.MTG_FLAG_COLUMN_KERNEL if column else 0))
    g, p, s = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    nat.check(lib.mtg_solve_ragged_plan(N, D, r, B, addr, flags, ctypes.byref(g), ctypes.byref(p), ctypes.byref(s)))
    return {"n_groups": g.value, "n_in_place": p.value, "total_segments": s.value}


def host_solve_linear_ragged_batch(N, r, values, mask, times, seg_count, free=False, n_free=False, cost=False,
                                   status=False, threads=1):
    """The library's host (CPU) path of Context.solve_linear_ragged_batch
    (mtg_host_solve_linear_ragged_batch): the same CSR arrays and outputs, no GPU.  Every trajectory's
    outputs are the bytes host_solve_linear_batch gives for it alone."""
    lib = nat.load()
    values = np.ascontiguousarray(values, dtype=np.float64)
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    times = np.ascontiguousarray(times, dtype=np.float64)
    seg_count = np.ascontiguousarray(seg_count, dtype=np.int32)
    B = int(seg_count.shape[0])
    totS = int(seg_count.sum(dtype=np.int64))
    totV = totS + B
    h = N // 2
    assert values.ndim == 3 and values.shape[1] == h, "values must be [sum V][N/2][D]"
    D = int(values.shape[2])
    assert values.shape[0] == totV and mask.shape == (totV,) and times.shape == (totS,)
    out = {"coeffs": np.empty((totS, D, N))}
    if free:
        out["free"] = np.empty((totV * h * D,))
    if n_free:
        out["n_free"] = np.empty((B,), np.int32)
    if cost:
        out["cost"] = np.empty((B,))
    if status:
        out["status"] = np.empty((B,), np.int32)
    nat.check(lib.mtg_host_solve_linear_ragged_batch(N, D, r, B, _addr(seg_count), _addr(values), _addr(mask),
                                                     _addr(times), _addr(out["coeffs"]), _addr(out.get("free")),
                                                     _addr(out.get("n_free")), _addr(out.get("cost")),
                                                     _addr(out.get("status")), threads))
    return out


def host_evaluate_at_ragged_batch(coeffs, times, seg_count, t_query, derivative_begin=0, n_derivatives=1,
                                  want_in_range=True, threads=0):
    """Context.evaluate_at_ragged_batch on the library's host path (mtg_host_evaluate_at_ragged_batch): no GPU;
    every trajectory's rows are the bytes host_evaluate_at_batch gives for it alone.  numpy CSR arrays (or lists
    of per-trajectory blocks, as split_ragged yields); threads <= 0: mtg_host_default_threads()."""
    coeffs = np.ascontiguousarray(_csr(coeffs), dtype=np.float64)
    times = np.ascontiguousarray(_csr(times), dtype=np.float64)
    seg_count, B, D, N = _ragged_coeff_shape(coeffs, times, seg_count)
    t_query, t_stride, M = _query_rows_numpy(t_query, B)
    out = np.empty((B, M, n_derivatives, D))
    in_range = np.empty((B, M), np.uint8) if want_in_range else None
    status = np.empty(B, np.int32)
    nat.check(nat.load().mtg_host_evaluate_at_ragged_batch(N, D, B, _addr(seg_count), _addr(coeffs), _addr(times),
                                                           _addr(t_query), t_stride, M, int(derivative_begin),
                                                           int(n_derivatives), _addr(out), _addr(in_range),
                                                           _addr(status), int(threads)))
    return out, in_range, status


def host_min_max_magnitude_ragged_batch(coeffs, times, seg_count, derivative, dimensions=None, threads=1):
    """Context.min_max_magnitude_ragged_batch on the library's host path
    (mtg_host_min_max_magnitude_ragged_batch): no GPU; every entry is the bytes host_min_max_magnitude_batch
    gives for that trajectory alone.  numpy CSR arrays (or lists of per-trajectory blocks)."""
    coeffs = np.ascontiguousarray(_csr(coeffs), dtype=np.float64)
    times = np.ascontiguousarray(_csr(times), dtype=np.float64)
    seg_count, B, D, N = _ragged_coeff_shape(coeffs, times, seg_count)
    mask = 0 if dimensions is None else int(sum(1 << int(d) for d in dimensions))
    mn = np.zeros(B, dtype=EXTREMUM_DTYPE)
    mx = np.zeros(B, dtype=EXTREMUM_DTYPE)
    nat.check(nat.load().mtg_host_min_max_magnitude_ragged_batch(N, D, B, _addr(seg_count), _addr(coeffs), _addr(times),
                                                                 int(derivative), mask, _addr(mn), _addr(mx),
                                                                 int(threads)))
    return mn, mx


def host_vertex_derivatives_batch(coeffs, times, threads=1):
    """Context.vertex_derivatives_batch on the library's host path (mtg_host_vertex_derivatives_batch): scalar
    C++, no GPU, any K.  coeffs [B][K][D][N], times [B][K] -> [B][K + 1][N/2][D]."""
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    B, K, D, N = coeffs.shape
    assert times.shape == (B, K)
    out = np.empty((B, K + 1, N // 2, D))
    nat.check(nat.load().mtg_host_vertex_derivatives_batch(N, D, K, B, _addr(coeffs), _addr(times), _addr(out),
                                                           int(threads)))
    return out


def host_vertex_derivatives_ragged_batch(coeffs, times, seg_count, threads=1):
    """Context.vertex_derivatives_ragged_batch on the library's host path
    (mtg_host_vertex_derivatives_ragged_batch): no GPU; every trajectory's rows are the bytes
    host_vertex_derivatives_batch gives for it alone.  numpy CSR arrays (or lists of per-trajectory blocks)."""
    coeffs = np.ascontiguousarray(_csr(coeffs), dtype=np.float64)
    times = np.ascontiguousarray(_csr(times), dtype=np.float64)
    seg_count, B, D, N = _ragged_coeff_shape(coeffs, times, seg_count)
    out = np.empty((coeffs.shape[0] + B, N // 2, D))
    nat.check(nat.load().mtg_host_vertex_derivatives_ragged_batch(N, D, B, _addr(seg_count), _addr(coeffs), _addr(times),
                                                                  _addr(out), int(threads)))
    return out


def host_coefficients_from_vertices_ragged_batch(N, vertex_values, times, seg_count, threads=1):
    """Context.coefficients_from_vertices_ragged_batch on the library's host path
    (mtg_host_coefficients_from_vertices_ragged_batch): no GPU; every trajectory's block is the bytes
    mtg_host_coefficients_from_vertices_batch gives for it alone.  numpy CSR arrays (or lists of blocks)."""
    vertex_values = np.ascontiguousarray(_csr(vertex_values), dtype=np.float64)
    times = np.ascontiguousarray(_csr(times), dtype=np.float64)
    seg_count, B, D = _ragged_vertex_shape(N, vertex_values, times, seg_count)
    out = np.empty((times.shape[0], D, N))
    nat.check(nat.load().mtg_host_coefficients_from_vertices_ragged_batch(N, D, B, _addr(seg_count), _addr(vertex_values),
                                                                          _addr(times), _addr(out), int(threads)))
    return out


def host_collision_cost_ragged_batch(N, vertex_values, times, seg_count, grid, params, mask=None, grad=False, threads=1):
    """Context.collision_cost_ragged_batch on the library's host path (mtg_host_collision_cost_ragged_batch): no
    GPU; every trajectory's outputs are the bytes host_collision_cost_batch gives for it alone.  Same arguments
    (numpy CSR arrays) and outputs."""
    vertex_values = np.ascontiguousarray(_csr(vertex_values), dtype=np.float64)
    times = np.ascontiguousarray(_csr(times), dtype=np.float64)
    seg_count, B, D = _ragged_vertex_shape(N, vertex_values, times, seg_count)
    totV, h = vertex_values.shape[0], N // 2
    assert not grad or mask is not None, "grad needs mask"
    mask = np.ascontiguousarray(mask, dtype=np.uint8) if mask is not None else None
    assert mask is None or mask.shape == (totV,), "mask must be [sum K + B]"
    out = {"cost": np.empty(B), "collision": np.empty(B, np.uint8), "n_evaluated": np.empty(B, np.int32),
           "status": np.empty(B, np.int32)}
    if grad:
        out["grad"] = np.zeros((totV * h * D,))
    g, keep = grid.native()
    nat.check(nat.load().mtg_host_collision_cost_ragged_batch(
        N, D, B, _addr(seg_count), _addr(vertex_values), _addr(mask) if grad else None, _addr(times), ctypes.byref(g),
        ctypes.byref(params.native()), _addr(out["cost"]), _addr(out.get("grad")), _addr(out["collision"]),
        _addr(out["n_evaluated"]), _addr(out["status"]), int(threads)))
    del keep
    return out


# ----------------------------------------------------------------- generators
def random_vertices_path_batch(N, D, K, batch, seed0=0, average_distance=5.0, max_derivative=4,
                               v_max=2.0, a_max=2.0, magic=6.5, threads=0):
    """The reference bench generator (src/polynomial_timing_evaluation.cpp:34-112), seeds seed0..seed0+B-1."""
    lib = nat.load()
    V, h = K + 1, N // 2
    values = np.zeros((batch, V, h, D))
    mask = np.zeros((batch, V), dtype=np.uint8)
    times = np.zeros((batch, K))
    nat.check(lib.mtg_host_random_vertices_path_batch(N, D, K, average_distance, max_derivative, seed0, batch,
                                                      v_max, a_max, magic, _addr(values), _addr(mask),
                                                      _addr(times), threads))
    return values, mask, times


def random_vertices_batch(N, D, K, batch, pos_min, pos_max, seed0=0, max_derivative=4, v_max=3.0, a_max=5.0,
                          magic=6.5, threads=0):
    """createRandomVertices + estimateSegmentTimes (src/vertex.cpp:27-79, :162-178)."""
    lib = nat.load()
    V, h = K + 1, N // 2
    pos_min = np.ascontiguousarray(pos_min, dtype=np.float64)
    pos_max = np.ascontiguousarray(pos_max, dtype=np.float64)
    assert len(pos_min) == D and len(pos_max) == D
    values = np.zeros((batch, V, h, D))
    mask = np.zeros((batch, V), dtype=np.uint8)
    times = np.zeros((batch, K))
    nat.check(lib.mtg_host_random_vertices_batch(N, D, K, max_derivative, _addr(pos_min), _addr(pos_max), seed0,
                                                 batch, v_max, a_max, magic, _addr(values), _addr(mask),
                                                 _addr(times), threads))
    return values, mask, times
