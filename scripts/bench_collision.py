#!/usr/bin/env python3
"""Collision cost + gradient throughput (include/mtg.h mtg_collision_cost_batch): 1e4 config-2
trajectories (K = 10, N = 10, D = 3) solved on the GPU, a 128^3 union-of-spheres distance field,
dt = 0.1, gradient on, everything device-resident.  Prints one JSON line: the kernel time (HIP events
in the dispatch packet, warmed, median of STEPS launches), samples per second, and the library's host
path on 16 threads for the same batch.

Run on the GPU box: python scripts/bench_collision.py"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mav_trajectory_generation_cmake_amd as mtg  # noqa: E402

B = int(os.environ.get("B", "10000"))
steps = max(20, int(os.environ.get("STEPS", "30")))
host_threads = int(os.environ.get("HOST_THREADS", "16"))
N, D, K, r = 10, 3, 10, 4

# the map: spheres over the volume the generator's paths cover
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
params = mtg.CollisionParams(0.1, 0.2, 1.0, 0.3, 2.0, (origin + 1.0,) * 3, (-origin - 1.0,) * 3, True)

vals, mask, times = mtg.random_vertices_path_batch(N, D, K, B, seed0=0)
ctx = mtg.Context(0)
sol = ctx.solve_linear_batch(N, r, vals, mask, times, free=True)
x = mtg.full_vertex_values(vals, mask, sol["free"], N)

dev = torch.device("cuda", 0)
x_d, t_d, m_d = (torch.from_numpy(a).to(dev) for a in (x, times, mask))
grid_d = mtg.SdfGrid(torch.from_numpy(field).to(dev), (origin,) * 3, res, 1.0)


def run():
    return ctx.collision_cost_batch(N, x_d, t_d, grid_d, params, mask=m_d, grad=True, asynchronous=True)


ctx.enable_timing(0)
for _ in range(5):
    out = run()
torch.cuda.synchronize()
ctx.enable_timing(steps)
for _ in range(steps):
    out = run()
ms = ctx.kernel_times_ms(steps)
torch.cuda.synchronize()
kernel_ms = float(np.median(ms))
evaluated = int(out["n_evaluated"].sum().item())
clock_samples = int(np.sum(np.ceil(times / 0.1)))

grid_h = mtg.SdfGrid(field, (origin,) * 3, res, 1.0)
host = None
host_s = []
for _ in range(3):
    t0 = time.perf_counter()
    host = mtg.host_collision_cost_batch(N, x, times, grid_h, params, mask=mask, grad=True, threads=host_threads)
    host_s.append(time.perf_counter() - t0)
host_ms = 1e3 * float(np.median(host_s))
cost_d = out["cost"].cpu().numpy()
agree = bool((out["n_evaluated"].cpu().numpy() == host["n_evaluated"]).all() and
             np.max(np.abs(cost_d - host["cost"]) / np.maximum(host["cost"], 1e-300)) < 1e-6)
print(json.dumps({
    "workload": "collision cost + gradient, config2 trajectories (K=10, N=10, D=3), 128^3 sphere map, dt=0.1",
    "B": B, "steps": steps, "kernel_ms": kernel_ms, "kernel_ms_min": float(np.min(ms)), "kernel_ms_max": float(np.max(ms)),
    "clock_samples": clock_samples, "evaluated_samples": evaluated,
    "clock_samples_per_s": clock_samples / (kernel_ms * 1e-3), "evaluated_samples_per_s": evaluated / (kernel_ms * 1e-3),
    "trajectories_per_s": B / (kernel_ms * 1e-3),
    "host_threads": host_threads, "host_ms": host_ms, "host_evaluated_samples_per_s": evaluated / (host_ms * 1e-3),
    "speedup_over_host": host_ms / kernel_ms, "device_agrees_with_host": agree}))
