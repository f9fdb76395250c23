#!/usr/bin/env python3
"""Segment-time gradient of the collision cost (include/mtg.h mtg_collision_time_gradient_batch):
1e4 config-2 trajectories (generator + solve, K = 10, N = 10, D = 3), a 128^3 union-of-spheres
distance field, dt = 0.1, map_resolution = 0.2, increment_time = 0.1, everything device-resident.

Prints one JSON line:
  kernel_ms            the new call (HIP events in the dispatch packet, warmed; median, min, max of STEPS
                       launches, alternated with yardstick (b) launch by launch)
  segments_walked      mean per trajectory, and the share of the perturbations that can rejoin (n+2 < K)
                       which did not walk to the end
  host_ms              yardstick (a): the library's host path on HOST_THREADS threads
  cost_batch_ms        yardstick (b): mtg_collision_cost_batch without gradient on the 2K B batch of
                       perturbed times.  It walks every segment of every perturbation with re-formed
                       coefficients: a time yardstick only, its values are something else.
  spread               (max - min) / median of each device timing, the run-to-run spread to hold a
                       difference against

Run on the GPU box: python scripts/bench_collision_time_gradient.py"""
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
host_B = min(B, int(os.environ.get("HOST_B", "2000")))  # the host path is timed on a slice and scaled
N, D, K, r = 10, 3, 10, 4
inc = 0.1

# the map of bench_collision.py: spheres over the volume the generator's paths cover
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

# yardstick (b)'s batch: for every trajectory its 2K perturbed time vectors
tp = np.repeat(times[:, None, :], 2 * K, axis=1)  # [B][2K][K]
for k in range(K):
    small = times[:, k] <= 0.1
    tp[:, 2 * k, k] = np.where(small, 0.1, times[:, k] - inc)
    tp[:, 2 * k + 1, k] = np.where(small, 0.1, times[:, k] + inc)
assert (tp > 0).all(), "a generated segment time is <= increment_time"
xp = np.repeat(x, 2 * K, axis=0)
tp = tp.reshape(B * 2 * K, K)

dev = torch.device("cuda", 0)
x_d, t_d, xp_d, tp_d = (torch.from_numpy(a).to(dev) for a in (x, times, xp, tp))
grid_d = mtg.SdfGrid(torch.from_numpy(field).to(dev), (origin,) * 3, res, 1.0)


def run_new():
    return ctx.collision_time_gradient_batch(N, x_d, t_d, grid_d, params, increment_time=inc, asynchronous=True)


def run_b():
    return ctx.collision_cost_batch(N, xp_d, tp_d, grid_d, params, asynchronous=True)


ctx.enable_timing(0)
for _ in range(5):
    out = run_new()
    run_b()
torch.cuda.synchronize()
ctx.enable_timing(2 * steps)
for _ in range(steps):  # alternated: both see the same machine
    out = run_new()
    run_b()
ms = np.array(ctx.kernel_times_ms(2 * steps))
torch.cuda.synchronize()
new_ms, b_ms = ms[0::2], ms[1::2]

walked = out["segments_walked"].cpu().numpy()
full = sum(2 * (K - k) for k in range(K))  # walked when nothing rejoins
least = 4 * K - 2                       # walked when everything rejoins at n+2
grid_h = mtg.SdfGrid(field, (origin,) * 3, res, 1.0)
host_s = []
for _ in range(3):
    t0 = time.perf_counter()
    host = mtg.host_collision_time_gradient_batch(N, x[:host_B], times[:host_B], grid_h, params, increment_time=inc,
                                                  threads=host_threads)
    host_s.append(time.perf_counter() - t0)
host_ms = 1e3 * float(np.median(host_s)) * B / host_B
sc = out["side_cost"].cpu().numpy()[:host_B]
agree = bool((out["side_evaluated"].cpu().numpy()[:host_B] == host["side_evaluated"]).all() and
             np.max(np.abs(sc - host["side_cost"]) / np.maximum(host["side_cost"], 1e-300)) < 1e-6)


# which perturbations rejoined: the early-stop rule restated by the tests' model, on a sample
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _collision_model as M  # noqa: E402
import _collision_time_model as TM  # noqa: E402

sample = range(0, B, max(1, B // int(os.environ.get("MODEL_SAMPLE", "48"))))
mgrid = M.Grid(field, (origin,) * 3, res, 1.0)
mprm = M.Params(0.1, 0.2, 1.0, 0.3, 2.0, (origin + 1.0,) * 3, (-origin - 1.0,) * 3, True)
can = at2 = later = never = 0
model_agrees = True
for j in sample:
    mdl = TM.model(N, x[j], times[j], mgrid, mprm, inc, truth=False)
    model_agrees &= mdl["segments_walked"] == int(walked[j])
    for (k, _), side in mdl["sides"].items():
        if k + 2 < K:
            can += 1
            at2 += side["rejoined"] and side["walked"] == 2
            later += side["rejoined"] and side["walked"] > 2
            never += not side["rejoined"]


def stats(v):
    med = float(np.median(v))
    return {"median": med, "min": float(np.min(v)), "max": float(np.max(v)), "spread": float((np.max(v) - np.min(v)) / med)}


print(json.dumps({
    "workload": "collision time gradient, config2 trajectories (K=10, N=10, D=3), 128^3 sphere map, dt=0.1, "
                "map_resolution=0.2, increment_time=0.1",
    "B": B, "steps": steps, "kernel_ms": stats(new_ms), "cost_batch_ms": stats(b_ms),
    "cost_batch_over_kernel": float(np.median(b_ms) / np.median(new_ms)),
    "segments_walked_mean": float(walked.mean()), "segments_walked_if_all_rejoin_at_n_plus_2": least,
    "segments_walked_if_none_rejoins": full,
    "share_of_trajectories_at_the_least": float((walked == least).mean()),
    "model_sample": len(sample), "model_walked_equals_device": bool(model_agrees),
    "perturbations_that_can_rejoin": int(can), "rejoined_at_n_plus_2": int(at2), "rejoined_later": int(later),
    "never_rejoined": int(never),
    "trajectories_per_s": B / (float(np.median(new_ms)) * 1e-3),
    "host_threads": host_threads, "host_trajectories_timed": host_B, "host_ms": host_ms,
    "host_over_kernel": host_ms / float(np.median(new_ms)), "device_agrees_with_host": agree}))
