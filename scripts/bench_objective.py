#!/usr/bin/env python3
"""One evaluation of the nonlinear objective (include/mtg.h mtg_objective_batch, objective 2 with soft
constraints and gradient) against the same evaluation composed from the five existing Python calls, on
the config-2 collision set-up of bench_collision_time_gradient.py (generator + solve, K = 10, N = 10,
D = 3, a 128^3 union-of-spheres field, dt = 0.1, map_resolution = 0.2, increment_time = 0.1), at
B = 1, 64 and 1e4.

  objective_device_ms   Context.objective_batch on device-resident tensors (x, values, mask, the grid,
                        the outputs), host clock from the call to the end of a device synchronise
  objective_host_ms     the same call on numpy arrays (staged in and out once each)
  composed_ms           what a caller does today from x on the host: unpack + full_vertex_values (a
                        Python loop over the batch), cost_at_times_batch, collision_cost_batch,
                        soft_constraint_cost_batch, time_jacobian_batch, collision_time_gradient_batch
                        on numpy arrays (each stages and synchronises), then the weighted sums and the
                        gather into x's layout in numpy
Each is the median of STEPS calls after WARMUP, the three alternated call by call so that they see
the same machine; spread = (max - min) / median.  The composed result must equal objective_batch's
cost and gradient bit for bit (asserted).  --compose-only times the composition alone and uses nothing
this call added to the package, so it also runs on a checkout without mtg_objective_batch (the baseline).

Run on the GPU box: python scripts/bench_objective.py [--compose-only]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mav_trajectory_generation_cmake_amd as mtg  # noqa: E402

compose_only = "--compose-only" in sys.argv
sizes = [int(b) for b in os.environ.get("SIZES", "1,64,10000").split(",")]
N, D, K, r = 10, 3, 10, 4
inc = 0.1
W = (0.1, 10.0, 1.0, 1.0)  # w_d, w_c, w_t, w_sc: the reference's defaults

n, res = 128, 0.25
origin = -0.5 * n * res
rng = np.random.default_rng(3)
centres = rng.uniform(origin + 1.0, -origin - 1.0, size=(96, 3))
radii = rng.uniform(0.5, 2.0, size=96)
ax = origin + (np.arange(n) + 0.5) * res
X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
field = np.full((n, n, n), np.inf, dtype=np.float64)
for c, rad in zip(centres, radii):
    np.minimum(field, np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - rad, out=field)
field = field.astype(np.float32)
cparams = mtg.CollisionParams(0.1, 0.2, 1.0, 0.3, 2.0, (origin + 1.0,) * 3, (-origin - 1.0,) * 3, True)
soft = mtg.SoftConstraintParams([(1, 3.0), (2, 5.0)], weight=5.0)
grid_h = mtg.SdfGrid(field, (origin,) * 3, res, 1.0)
ctx = mtg.Context(0)
dev = torch.device("cuda", 0)


def stats(v):
    v = 1e3 * np.asarray(v)
    med = float(np.median(v))
    return {"median": med, "min": float(v.min()), "max": float(v.max()), "spread": float((v.max() - v.min()) / med)}


def measure(B):
    vals, mask, times = mtg.random_vertices_path_batch(N, D, K, B, seed0=0)
    sol = ctx.solve_linear_batch(N, r, vals, mask, times, free=True, n_free=True)
    nf = sol["n_free"]
    assert (nf == nf[0]).all()  # the generator's pattern: the same n_free everywhere
    nf = int(nf[0])
    stride = K + D * nf
    x = np.zeros((B, stride))
    x[:, :K] = times
    x[:, K:] = sol["free"][:, :, :nf].reshape(B, D * nf)
    ones = np.ones((1, K))

    def composed():
        t = np.ascontiguousarray(x[:, :K])
        free = np.zeros((B, D, (K + 1) * (N // 2)))
        free[:, :, :nf] = x[:, K:].reshape(B, D, nf)
        full = mtg.full_vertex_values(vals, mask, free, N)
        Jd, gd = ctx.cost_at_times_batch(N, r, full, t, ones, mask=mask, grad=True)
        cc = ctx.collision_cost_batch(N, full, t, grid_h, cparams, mask=mask, grad=True)
        sc = ctx.soft_constraint_cost_batch(N, full, t, soft, mask=mask, grad=True)
        _, jd = ctx.time_jacobian_batch(N, r, full, t, ones, increment_time=inc)
        ct = ctx.collision_time_gradient_batch(N, full, t, grid_h, cparams, increment_time=inc, diagnostics=False)
        J_t = np.zeros(B)
        for i in range(K):
            J_t = J_t + t[:, i]
        cost = ((W[0] * Jd[:, 0] + W[1] * cc["cost"]) + W[2] * J_t) + W[3] * sc["cost"]
        g = np.empty((B, stride))
        g[:, :K] = ((W[0] * jd[:, 0] + W[1] * ct["grad_t"]) + W[3] * 0.0) + W[2]
        g[:, K:] = ((W[0] * gd[:, 0, :, :nf] + W[1] * cc["grad"][:, :, :nf]) + W[3] * sc["grad"][:, :, :nf]).reshape(B, D * nf)
        return cost, g

    runs = {"composed_ms": composed}
    if not compose_only:
        prm = mtg.ObjectiveParams(2, r, *W, increment_time=inc, use_soft_constraints=True)
        t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        grid_d = mtg.SdfGrid(t_(field), (origin,) * 3, res, 1.0)
        vals_d, mask_d, x_d = t_(vals), t_(mask), t_(x)

        def objective_device():
            out = ctx.objective_batch(N, vals_d, mask_d, x_d, prm, grid=grid_d, collision=cparams, soft=soft,
                                      asynchronous=True)
            torch.cuda.synchronize(dev)
            return out

        def objective_host():
            return ctx.objective_batch(N, vals, mask, x, prm, grid=grid_h, collision=cparams, soft=soft)

        runs = {"objective_device_ms": objective_device, "objective_host_ms": objective_host, "composed_ms": composed}
        cost, g = composed()
        for out in (objective_host(), {k: (v.cpu().numpy() if v is not None else None) for k, v in objective_device().items()
                                       if k != "state"}):
            assert (out["status"] == 0).all()
            assert out["cost"].tobytes() == cost.tobytes() and out["grad"].tobytes() == g.tobytes(), \
                "objective_batch and the composition differ"
    steps = int(os.environ.get("STEPS", "15" if B >= 5000 else "60"))
    warmup = int(os.environ.get("WARMUP", "3" if B >= 5000 else "10"))
    for _ in range(warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize(dev)
    took = {k: [] for k in runs}
    for _ in range(steps):  # alternated call by call
        for k, f in runs.items():
            t0 = time.perf_counter()
            f()
            took[k].append(time.perf_counter() - t0)
    res_ = {"B": B, "steps": steps, "warmup": warmup, "x_stride": stride}
    res_.update({k: stats(v) for k, v in took.items()})
    if not compose_only:
        res_["composed_over_objective_device"] = res_["composed_ms"]["median"] / res_["objective_device_ms"]["median"]
        res_["composed_over_objective_host"] = res_["composed_ms"]["median"] / res_["objective_host_ms"]["median"]
    return res_


print(json.dumps({
    "workload": "objective 2 (free constraints + collision + time) with soft constraints and gradient, config2 "
                "trajectories (K=10, N=10, D=3), 128^3 sphere map, dt=0.1, map_resolution=0.2, increment_time=0.1",
    "compose_only": compose_only,
    "kernel_launches_per_objective_call": 7, "kernel_launches_per_composition": 5,
    "sizes": [measure(B) for B in sizes]}))
ctx.close()
