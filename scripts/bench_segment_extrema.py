#!/usr/bin/env python3
"""Per-segment extrema throughput (include/mtg.h mtg_segment_min_max_magnitude_batch,
mtg_segment_min_max_axis_batch) against the whole-trajectory entry on the same batch.

Workload: B config-2 trajectories (K = 10, N = 10, D = 3; B = 1e4 is 1e5 segments) solved on the GPU,
derivative 1 and 2, every array device-resident.  Yardstick: mtg_min_max_magnitude_batch, which runs the
same per-segment search plus a reduction over the trajectory.  Variants: the magnitude entry, the axis
entry (3 items per segment, a much shorter root polynomial), the magnitude entry with the candidate list.
Each round launches the yardstick and every variant once, in turn, each between its own pair of HIP events
on one stream; the medians and the 10th / 90th percentiles over the rounds are reported.  Writes
profiles/segment_extrema_timing.json when OUT is set, and prints the same JSON.

Run on the GPU box: [B=10000 ROUNDS=300 OUT=profiles/segment_extrema_timing.json] python scripts/bench_segment_extrema.py"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mav_trajectory_generation_cmake_amd as mtg  # noqa: E402
from mav_trajectory_generation_cmake_amd import _native as nat  # noqa: E402
from mav_trajectory_generation_cmake_amd.solver import EXTREMUM_DTYPE, _addr  # noqa: E402

B = int(os.environ.get("B", "10000"))
rounds = int(os.environ.get("ROUNDS", "300"))
CAP = 8
N, D, K, r = 10, 3, 10, 4
S = B * K
vals, mask, times = mtg.random_vertices_path_batch(N, D, K, B, seed0=0)
ctx = mtg.Context(0)
coeffs = ctx.solve_linear_batch(N, r, vals, mask, times)["coeffs"]
dev = torch.device("cuda", 0)
c_d = torch.from_numpy(coeffs).to(dev)
t_d = torch.from_numpy(times).to(dev)
E = EXTREMUM_DTYPE.itemsize


def buf(n, dtype=torch.uint8):
    return torch.empty(n, dtype=dtype, device=dev)


umn, umx = buf(E * B), buf(E * B)
smn, smx = buf(E * S), buf(E * S)
amn, amx = buf(E * S * D), buf(E * S * D)
cand, cnt = buf(S * CAP, torch.float64), buf(S, torch.int32)
lib = ctx._lib
stream = torch.cuda.current_stream(dev)
ctx.set_stream(stream.cuda_stream)
ctx.enable_timing(0)
F = nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC
h = ctx.handle


def variants(k):
    return {
        "uniform_trajectory_entry": lambda: lib.mtg_min_max_magnitude_batch(h, N, D, K, B, _addr(c_d), _addr(t_d), k, 0,
                                                                            _addr(umn), _addr(umx), F),
        "segment_magnitude": lambda: lib.mtg_segment_min_max_magnitude_batch(
            h, N, D, S, _addr(c_d), _addr(t_d), None, k, 0, _addr(smn), _addr(smx), None, None, 0, None, F),
        "segment_axis": lambda: lib.mtg_segment_min_max_axis_batch(
            h, N, D, S, _addr(c_d), _addr(t_d), None, k, _addr(amn), _addr(amx), None, None, 0, None, F),
        "segment_magnitude_with_list": lambda: lib.mtg_segment_min_max_magnitude_batch(
            h, N, D, S, _addr(c_d), _addr(t_d), None, k, 0, _addr(smn), _addr(smx), _addr(cand), _addr(cnt), CAP,
            None, F),
    }


res = {"B": B, "segments": S, "rounds": rounds, "candidate_capacity": CAP,
       "workload": "config-2 trajectories (K=10, N=10, D=3), device-resident; ms per launch between HIP events, "
                   "launches of the four entries alternated round by round"}
for k in (1, 2):
    runs = variants(k)
    for _ in range(10):  # warm up every shape of the timed window
        for f in runs.values():
            nat.check(f(), h)
    torch.cuda.synchronize()
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)]
          for name in runs}
    for i in range(rounds):
        for name, f in runs.items():
            a, b = ev[name][i]
            a.record(stream)
            nat.check(f(), h)
            b.record(stream)
    torch.cuda.synchronize()
    out = {}
    for name in runs:
        ms = np.array([a.elapsed_time(b) for a, b in ev[name]])
        out[name] = {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)),
                     "p90_ms": float(np.percentile(ms, 90)), "segments_per_s": S / (float(np.median(ms)) * 1e-3)}
    # the results are the yardstick's: reduce the per-segment extremes with its rule
    sm = np.frombuffer(smx.cpu().numpy().tobytes(), dtype=EXTREMUM_DTYPE).reshape(B, K)
    um = np.frombuffer(umx.cpu().numpy().tobytes(), dtype=EXTREMUM_DTYPE)
    assert np.array_equal(sm["value"].max(axis=1), um["value"]), "per-segment maxima do not reduce to the trajectory's"
    res["derivative_%d" % k] = out
text = json.dumps(res, indent=1)
print(text)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        f.write(text + "\n")
ctx.close()
