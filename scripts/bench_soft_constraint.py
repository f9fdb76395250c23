#!/usr/bin/env python3
"""Soft-constraint cost + gradient (include/mtg.h mtg_soft_constraint_cost_batch): 1e4 config-2
trajectories (K = 10, N = 10, D = 3, 36 free derivatives per dimension) with limits on velocity and
acceleration, event-timed three ways in one run:

* kernel: mtg_soft_constraint_cost_batch with the gradient, device-resident arrays;
* composition: what the library offered before it -- the 2 D n_free + 1 = 217 perturbed copies of
  the batch, each through mtg_coefficients_from_vertices_batch and one mtg_min_max_magnitude_batch per
  constraint (one copy of the batch per chunk); the SUM of the kernel times, staging not counted;
* host: mtg_host_soft_constraint_cost_batch (the reference loop written literally) on 16 threads, on
  the first HOST_B trajectories and scaled to B (the literal loop is ~430 whole-trajectory searches
  per trajectory).

Prints one JSON line.  Kernel times are HIP events in the dispatch packet, warmed, median of STEPS
launches with min / max; the composition is timed REPS times over all copies.

Run on the GPU box: python scripts/bench_soft_constraint.py"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mav_trajectory_generation_cmake_amd as mtg  # noqa: E402

B = int(os.environ.get("B", "10000"))
steps = max(10, int(os.environ.get("STEPS", "20")))
reps = max(1, int(os.environ.get("REPS", "1")))
host_threads = int(os.environ.get("HOST_THREADS", "16"))
host_b = min(B, int(os.environ.get("HOST_B", "320")))
N, D, K, r = 10, 3, 10, 4
inc = 0.05

vals, mask, times = mtg.random_vertices_path_batch(N, D, K, B, seed0=0)
ctx = mtg.Context(0)
sol = ctx.solve_linear_batch(N, r, vals, mask, times, free=True)
x = mtg.full_vertex_values(vals, mask, sol["free"], N)
coeffs = ctx.coefficients_from_vertices_batch(N, x, times)
limits = [(k, 0.8 * float(np.median(ctx.min_max_magnitude_batch(coeffs, times, k)[1]["value"]))) for k in (1, 2)]
params = mtg.SoftConstraintParams(limits, weight=10.0, increment=inc)

dev = torch.device("cuda", 0)
x_d, t_d, m_d = (torch.from_numpy(a).to(dev) for a in (x, times, mask))


def run():
    return ctx.soft_constraint_cost_batch(N, x_d, t_d, params, mask=m_d, grad=True, asynchronous=True)


ctx.enable_timing(0)
for _ in range(3):
    out = run()
torch.cuda.synchronize()
ctx.enable_timing(steps)
for _ in range(steps):
    out = run()
ms = ctx.kernel_times_ms(steps)
torch.cuda.synchronize()
kernel_ms = float(np.median(ms))
result = {
    "workload": "soft-constraint cost + gradient, config2 trajectories (K=10, N=10, D=3), limits on v and a",
    "B": B, "steps": steps, "kernel_ms": kernel_ms, "kernel_ms_min": float(np.min(ms)), "kernel_ms_max": float(np.max(ms)),
    "trajectories_per_s": B / (kernel_ms * 1e-3)}
# the composition: every perturbed copy of the batch, one copy per chunk
h, V = N // 2, K + 1
slots = [(v, k) for v in range(V) for k in range(h) if not (int(mask[0, v]) >> k) & 1]
assert (mask == mask[0]).all() and len(slots) == 36
copies = [None] + [(v, k, d, s) for d in range(D) for (v, k) in slots for s in (-inc, inc)]
ctx.enable_timing(1)


def composition():
    total = 0.0
    for pert in copies:
        xp = x
        if pert is not None:
            v, k, d, s = pert
            xp = x.copy()
            xp[:, v, k, d] += s
        c = ctx.coefficients_from_vertices_batch(N, xp, times)
        total += float(ctx.kernel_times_ms(1)[-1])
        for kk, _ in limits:
            ctx.min_max_magnitude_batch(c, times, kk)
            total += float(ctx.kernel_times_ms(1)[-1])
    return total


composition_ms = [composition() for _ in range(reps + 1)][1:]  # (the first pass warms up)

host_s = []
for _ in range(2):
    t0 = time.perf_counter()
    host = mtg.host_soft_constraint_cost_batch(N, x[:host_b], times[:host_b], params, mask=mask[:host_b], grad=True,
                                               threads=host_threads)
    host_s.append(time.perf_counter() - t0)
host_ms = 1e3 * float(np.min(host_s)) * B / host_b
# a sanity check that the two paths computed the same thing (relative 1e-6 of the cost and of each
# trajectory's largest gradient entry), NOT the derived tolerance: that is tests/_soft_constraint_model.py.
# (The limits are 0.8 x the batch's median maximum, so about half of the trajectories do not violate
# them; the work does not depend on that.)
g_d, c_d = out["grad"].cpu().numpy()[:host_b], out["cost"].cpu().numpy()[:host_b]
scale = np.maximum(np.abs(host["grad"]).max(axis=(1, 2), keepdims=True), 1e-300)
agree = bool(np.max(np.abs(c_d - host["cost"]) / host["cost"]) < 1e-6 and np.max(np.abs(g_d - host["grad"]) / scale) < 1e-6)
comp = float(np.median(composition_ms))
result.update({
    "composition_copies": len(copies), "composition_kernel_ms": comp, "composition_kernel_ms_runs": composition_ms,
    "host_threads": host_threads, "host_trajectories": host_b, "host_ms_scaled_to_B": host_ms,
    "speedup_over_composition": comp / kernel_ms, "speedup_over_host": host_ms / kernel_ms,
    "device_agrees_with_host": agree})
print(json.dumps(result))
