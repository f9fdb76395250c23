#!/usr/bin/env python3
"""mtg_evaluate_at_batch throughput: solved config-2 coefficients, B = 1e4, device-
resident; M in {1, 16, 256} query times per trajectory x n_derivatives in {1, 3}.  Every launch is
event-timed (the events ride in the kernel's dispatch packet) after a time-based warm-up; the median of
STEPS launches is reported.  The outputs rotate over distinct buffers -- at least 512 MB of them where 64
buffers reach that -- so the larger cases cannot sit in the 256 MB Infinity Cache (the small ones do: their
whole output is under a megabyte per launch, and the figures say so).  In the same session
mtg_evaluate_range_batch_full runs at a dt that gives about the samples of M = 256, for the time per
sample of both.  Prints one JSON line per case and one summary line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mav_trajectory_generation_cmake_amd as mtg  # noqa: E402
from mav_trajectory_generation_cmake_amd import _native as nat  # noqa: E402
from mav_trajectory_generation_cmake_amd.solver import _addr  # noqa: E402

B = int(os.environ.get("B", "10000"))
STEPS = max(30, int(os.environ.get("STEPS", "40")))
WARM_S = float(os.environ.get("WARM_S", "0.3"))
WRITE_CEILING = 5.5e12  # plain-store write ceiling of DESIGN.md (5.4-5.6 TB/s measured)
ROTATE_BYTES = 512 << 20
N, D, K, r = 10, 3, 10, 4

vals, mask, times = mtg.random_vertices_path_batch(N, D, K, B, seed0=0)
ctx = mtg.Context(0)
coeffs = ctx.solve_linear_batch(N, r, vals, mask, times)["coeffs"]
dev = torch.device("cuda", 0)
c_d = torch.from_numpy(coeffs).to(dev)
t_d = torch.from_numpy(times).to(dev)
lib = ctx._lib
ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
F = nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC
ctx.enable_timing(STEPS)
total_time = times.sum(axis=1)
rng = np.random.default_rng(0)


def timed(fn):
    """median of STEPS event-timed launches (ms) after WARM_S seconds of launches"""
    t0 = time.perf_counter()
    i = 0
    while time.perf_counter() - t0 < WARM_S:
        fn(i)
        i += 1
        if i % 16 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    for j in range(STEPS):
        fn(i + j)
    torch.cuda.synchronize()
    ms = ctx.kernel_times_ms(STEPS)
    assert len(ms) == STEPS
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


cases = []
for M in (1, 16, 256):
    tq = rng.uniform(0.0, 1.0, size=(B, M)) * total_time[:, None]
    q_d = torch.from_numpy(tq).to(dev)
    for nd in (1, 3):
        out_bytes = B * M * nd * D * 8
        n_buf = int(min(64, max(2, -(-ROTATE_BYTES // out_bytes))))
        outs = [torch.empty((B, M, nd, D), dtype=torch.float64, device=dev) for _ in range(n_buf)]
        inr = [torch.empty((B, M), dtype=torch.uint8, device=dev) for _ in range(n_buf)]
        st_d = torch.empty(B, dtype=torch.int32, device=dev)

        def run(i, M=M, nd=nd, outs=outs, inr=inr, q_d=q_d, st_d=st_d):
            k = i % len(outs)
            nat.check(lib.mtg_evaluate_at_batch(ctx.handle, N, D, K, B, _addr(c_d), _addr(t_d), _addr(q_d), M, M, 0, nd,
                                                _addr(outs[k]), _addr(inr[k]), _addr(st_d), F), ctx.handle)

        med, lo, hi = timed(run)
        # one launch's result against the host path, all rows
        want = mtg.host_evaluate_at_batch(coeffs, times, tq, 0, nd)[0]
        got = outs[0].cpu().numpy()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (M, nd)
        path = nat.evaluate_at_path(N, D, K, M, nd)
        rate = out_bytes / (med * 1e-3)
        # the bytes the algorithm needs: the output, in_range, the query times, the times, and the
        # coefficients a query needs (its segment's D N; the staged kernel reads all K D N once per block)
        read = B * M * 8 + B * K * 8 + (B * K * D * N * 8 if path == nat.MTG_EVALUATE_AT_STAGED else B * M * D * N * 8)
        case = {"M": M, "n_derivatives": nd, "path": "staged" if path == nat.MTG_EVALUATE_AT_STAGED else "lane",
                "us_per_launch": med * 1e3, "us_min": lo * 1e3, "us_max": hi * 1e3, "out_bytes": out_bytes,
                "out_TBps": rate / 1e12, "frac_write_ceiling": rate / WRITE_CEILING, "rotated_buffers": n_buf,
                "rotated_MB": n_buf * out_bytes / 2**20, "algorithmic_bytes": out_bytes + B * M + read,
                "ns_per_sample": med * 1e6 / (B * M)}
        cases.append(case)
        print(json.dumps(case), flush=True)
        del outs, inr

# range sampling at about the samples of M = 256 (one order per call, samples + sample times)
dt = float(total_time.mean() / 256.0)
t_end = 1e9
cap = mtg.solver.evaluate_range_capacity(times, 0.0, t_end, dt)
n_buf = int(min(64, max(2, -(-ROTATE_BYTES // (cap * (D + 1) * 8)))))
fc_d = torch.empty(B, dtype=torch.int64, device=dev)
fo_d = torch.empty(B, dtype=torch.int64, device=dev)
ft_d = torch.zeros(1, dtype=torch.int64, device=dev)
fouts = [torch.empty((cap, D), dtype=torch.float64, device=dev) for _ in range(n_buf)]
fsts = [torch.empty(cap, dtype=torch.float64, device=dev) for _ in range(n_buf)]


def full(i):
    k = i % n_buf
    nat.check(lib.mtg_evaluate_range_batch_full(ctx.handle, N, D, K, B, _addr(c_d), _addr(t_d), 0.0, t_end, dt, 0,
                                                _addr(fc_d), _addr(fo_d), _addr(ft_d), _addr(fouts[k]), _addr(fsts[k]),
                                                cap, F), ctx.handle)


# the range call launches several kernels: its time is the wall time of a synchronised window
for i in range(8):
    full(i)
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(STEPS):
    full(i)
torch.cuda.synchronize()
range_ms = (time.perf_counter() - t0) / STEPS * 1e3
samples = int(ft_d.item())
m256 = next(c for c in cases if c["M"] == 256 and c["n_derivatives"] == 1)
print(json.dumps({"B": B, "steps": STEPS, "cases": cases,
                  "range_full": {"dt": dt, "samples": samples, "samples_per_traj": samples / B, "ms_per_call_wall": range_ms,
                                 "ns_per_sample": range_ms * 1e6 / samples, "rotated_buffers": n_buf,
                                 "note": "wall time per call over a synchronised window of STEPS asynchronous calls "
                                         "(three kernels per call); samples and sample times written"},
                  "evaluate_at_M256_ns_per_sample": m256["ns_per_sample"],
                  "note": "evaluate_at: median of event-timed launches, outputs rotated over rotated_buffers buffers"}))
