#!/usr/bin/env python3
"""Cost of the ragged evaluate_at and min / max magnitude (mtg_evaluate_at_ragged_batch,
mtg_min_max_magnitude_ragged_batch) against the uniform calls they replace.  The shape of
scripts/timing_ragged.py: 1e4 trajectories, N = 10, D = 3, K uniform over {5, ..., 15}, solved
coefficients, device-resident arrays; times are device events (mtg_kernel_times: a call's first to its
last kernel).  A ragged call's host work and its upload of the segment offsets or plan records come
before its first kernel and are in none of the figures.

  (a) uniform   the sum over K of one uniform call per K-group on packed arrays: the baseline.  It leaves
                out the bucketing copies a caller of the uniform entries needs for an unsorted batch.
  (b) sorted    one ragged call on the batch sorted by K
  (c) shuffled  one ragged call on the shuffled batch

evaluate_at: M in {1, 16, 256} query times per trajectory x n_derivatives in {1, 3}; (b) and (c) read the
coefficients where they lie (8 (B + 1) more bytes: the offsets).  min / max magnitude (derivative 1, all
dimensions): (b) runs the kernels of (a) on the same bytes, (c) adds the coefficient gather -- 8 (K D N + K)
bytes per trajectory read and written -- and the scatter of the results.

Every shape is warmed up, then the three cases are taken in turn inside each of REPS repetitions, the
outputs rotating over distinct buffers; the median and the 10th to 90th percentile are reported, and the
timed calls' outputs are compared with the uniform calls' afterwards.  The GPU work runs in a child
process under a time limit; if it fails or times out nothing is written.  Writes
profiles/evaluate_ragged_timing.json.  Needs a HIP device."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "evaluate_ragged_timing.json")
N, D, R, B = 10, 3, 4, 10000
KS = tuple(range(5, 16))
MS, NDS = (1, 16, 256), (1, 3)
WARMUP, REPS = 10, 60
ROTATE_BYTES = 512 << 20
COPY_RATE = 6.3e12  # the copy rate DESIGN.md 3.14 uses
STEP_LIMIT_S = 420


def measure():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import mav_trajectory_generation_cmake_amd as mtg
    from mav_trajectory_generation_cmake_amd import _native as nat
    from mav_trajectory_generation_cmake_amd.solver import EXTREMUM_DTYPE, _addr

    rng = np.random.default_rng(2024)
    ks = rng.choice(KS, size=B)
    counts = {int(K): int((ks == K).sum()) for K in KS}
    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)
    lib = ctx._lib
    coeffs, times = {}, {}
    for K in KS:
        v, m, t = mtg.random_vertices_path_batch(N, D, K, counts[K], seed0=1000 * K)
        coeffs[K], times[K] = ctx.solve_linear_batch(N, R, v, m, t)["coeffs"], t

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    sorted_order = [(K, i) for K in KS for i in range(counts[K])]
    shuffled = [sorted_order[j] for j in rng.permutation(B)]
    # row of the sorted batch for every row of the shuffled one
    first = dict(zip(KS, np.concatenate([[0], np.cumsum([counts[K] for K in KS])])))
    to_sorted = to_dev(np.array([first[K] + i for K, i in shuffled], dtype=np.int64))
    total = np.concatenate([times[K].sum(axis=1) for K in KS])  # sorted order
    g_c = {K: to_dev(coeffs[K]) for K in KS}
    g_t = {K: to_dev(times[K]) for K in KS}

    def csr(order):
        c = to_dev(np.concatenate([coeffs[K][i] for K, i in order]))
        t = to_dev(np.concatenate([times[K][i] for K, i in order]))
        return c, t, np.array([K for K, _ in order], dtype=np.int32)

    c_b, t_b, seg_b = csr(sorted_order)
    c_c, t_c, seg_c = csr(shuffled)
    tot_s = int(seg_b.sum())
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    F = nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC
    ctx.enable_timing(16)
    n_a = len(KS)

    def stats(x):
        return {"median_us": round(float(np.median(x)) * 1e3, 2), "p10_us": round(float(np.percentile(x, 10)) * 1e3, 2),
                "p90_us": round(float(np.percentile(x, 90)) * 1e3, 2)}

    def run_case(uniform, call_b, call_c, n_buf):
        rows = []
        for rep in range(WARMUP + REPS):
            k = rep % n_buf
            for K in KS:
                uniform(K, k)
            call_b(k)
            call_c(k)
            ms = ctx.kernel_times_ms(n_a + 2)      # synchronizes
            assert len(ms) == n_a + 2
            if rep >= WARMUP:
                rows.append((float(ms[:n_a].sum()), float(ms[n_a]), float(ms[n_a + 1])))
        a = np.array(rows)
        res = {"a_uniform_sum": stats(a[:, 0]), "b_ragged_sorted": stats(a[:, 1]), "c_ragged_shuffled": stats(a[:, 2]),
               "b_over_a": round(float(np.median(a[:, 1]) / np.median(a[:, 0])), 4),
               "c_over_a": round(float(np.median(a[:, 2]) / np.median(a[:, 0])), 4), "rotated_buffers": n_buf}
        p10, p90 = res["a_uniform_sum"]["p10_us"], res["a_uniform_sum"]["p90_us"]
        for key in ("b_ragged_sorted", "c_ragged_shuffled"):
            res[key]["within_a_spread"] = bool(res[key]["median_us"] <= p90)
        res["a_spread_us"] = [p10, p90]
        return res, a

    def same_bits(x, y):
        x, y = x.contiguous().view(torch.int64).reshape(-1), y.contiguous().view(torch.int64).reshape(-1)
        return bool((x == y).all())

    result = {"shape": {"N": N, "D": D, "batch": B, "K": [KS[0], KS[-1]], "counts": counts, "total_segments": tot_s},
              "reps": REPS, "warmup": WARMUP, "evaluate_at": [], "offset_bytes": 8 * (B + 1)}

    # ------------------------------------------------------------------ evaluate_at
    for M in MS:
        tq = rng.uniform(0.0, 1.0, size=(B, M)) * total[:, None]          # sorted order
        q_b = to_dev(tq)
        q_c = q_b[to_sorted].contiguous()
        q_g, b0 = {}, 0
        for K in KS:
            q_g[K] = q_b[b0:b0 + counts[K]].contiguous()
            b0 += counts[K]
        for nd in NDS:
            W = nd * D
            out_bytes = B * M * W * 8
            n_buf = int(min(6, max(2, -(-ROTATE_BYTES // out_bytes))))
            o_a = [{K: torch.empty((counts[K], M, nd, D), dtype=torch.float64, device=dev) for K in KS} for _ in range(n_buf)]
            o_b = [torch.empty((B, M, nd, D), dtype=torch.float64, device=dev) for _ in range(n_buf)]
            o_c = [torch.empty((B, M, nd, D), dtype=torch.float64, device=dev) for _ in range(n_buf)]
            r_a = {K: torch.empty((counts[K], M), dtype=torch.uint8, device=dev) for K in KS}
            r_b, r_c = (torch.empty((B, M), dtype=torch.uint8, device=dev) for _ in range(2))
            s_a = {K: torch.empty(counts[K], dtype=torch.int32, device=dev) for K in KS}
            s_b, s_c = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))

            def uniform(K, k):
                nat.check(lib.mtg_evaluate_at_batch(ctx.handle, N, D, K, counts[K], _addr(g_c[K]), _addr(g_t[K]),
                                                    _addr(q_g[K]), M, M, 0, nd, _addr(o_a[k][K]), _addr(r_a[K]),
                                                    _addr(s_a[K]), F), ctx.handle)

            def ragged(c, t, seg, q, outs, inr, st):
                def call(k):
                    nat.check(lib.mtg_evaluate_at_ragged_batch(ctx.handle, N, D, B, _addr(seg), _addr(c), _addr(t), _addr(q),
                                                               M, M, 0, nd, _addr(outs[k]), _addr(inr), _addr(st), F),
                              ctx.handle)
                return call

            res, _ = run_case(uniform, ragged(c_b, t_b, seg_b, q_b, o_b, r_b, s_b),
                              ragged(c_c, t_c, seg_c, q_c, o_c, r_c, s_c), n_buf)
            torch.cuda.synchronize()
            want = torch.cat([o_a[0][K] for K in KS])
            assert same_bits(o_b[0], want), ("sorted", M, nd)
            assert same_bits(o_c[0], want[to_sorted]), ("shuffled", M, nd)
            assert bool((r_c == torch.cat([r_a[K] for K in KS])[to_sorted]).all())
            path = nat.evaluate_at_ragged_path(N, D, KS[-1], M, nd)
            paths_a = sorted({nat.evaluate_at_path(N, D, K, M, nd) for K in KS})
            res.update({"M": M, "n_derivatives": nd, "out_bytes": out_bytes,
                        "ragged_path": "staged" if path == nat.MTG_EVALUATE_AT_STAGED else "lane",
                        "uniform_paths": ["staged" if p == nat.MTG_EVALUATE_AT_STAGED else "lane" for p in paths_a]})
            result["evaluate_at"].append(res)
            print(json.dumps(res), file=sys.stderr, flush=True)
            del o_a, o_b, o_c

    # ------------------------------------------------------------ min / max magnitude
    esz = EXTREMUM_DTYPE.itemsize
    n_buf = 4
    mn_a = [{K: torch.zeros((counts[K], esz), dtype=torch.uint8, device=dev) for K in KS} for _ in range(n_buf)]
    mx_a = [{K: torch.zeros((counts[K], esz), dtype=torch.uint8, device=dev) for K in KS} for _ in range(n_buf)]
    mn_b, mx_b, mn_c, mx_c = ([torch.zeros((B, esz), dtype=torch.uint8, device=dev) for _ in range(n_buf)] for _ in range(4))

    def mm_uniform(K, k):
        nat.check(lib.mtg_min_max_magnitude_batch(ctx.handle, N, D, K, counts[K], _addr(g_c[K]), _addr(g_t[K]), 1, 0,
                                                  _addr(mn_a[k][K]), _addr(mx_a[k][K]), F), ctx.handle)

    def mm_ragged(c, t, seg, mn, mx):
        def call(k):
            nat.check(lib.mtg_min_max_magnitude_ragged_batch(ctx.handle, N, D, B, _addr(seg), _addr(c), _addr(t), 1, 0,
                                                             _addr(mn[k]), _addr(mx[k]), F), ctx.handle)
        return call

    res, a = run_case(mm_uniform, mm_ragged(c_b, t_b, seg_b, mn_b, mx_b), mm_ragged(c_c, t_c, seg_c, mn_c, mx_c), n_buf)
    torch.cuda.synchronize()
    for got_b, got_c, per_k in ((mn_b[0], mn_c[0], mn_a[0]), (mx_b[0], mx_c[0], mx_a[0])):
        want = torch.cat([per_k[K] for K in KS])
        assert bool((got_b == want).all()), "sorted"
        assert bool((got_c == want[to_sorted]).all()), "shuffled"
    gather_bytes = 2 * 8 * (tot_s * D * N + tot_s)
    c_minus_b = float(np.median(a[:, 2] - a[:, 1])) * 1e3
    res["gather"] = {"bytes_read_and_written": gather_bytes, "us_at_copy_rate": round(gather_bytes / COPY_RATE * 1e6, 2),
                     "copy_rate_TB_per_s": COPY_RATE / 1e12, "c_minus_b_us": round(c_minus_b, 2),
                     "us_at_copy_rate_over_c_minus_b": round(gather_bytes / COPY_RATE * 1e6 / max(c_minus_b, 1e-9), 3),
                     "note": "c - b also holds the scatter of the results, two more launches and the extrema launches "
                             "on the packed arrays: this ratio is not the gather kernel's share of the copy rate, "
                             "which needs the kernel's own time (a kernel trace, DESIGN.md 3.15)"}
    res.update({"derivative": 1, "dimensions": "all"})
    result["min_max_magnitude"] = res
    ctx.close()
    print(json.dumps(result), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        measure()
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child"],
                       capture_output=True, text=True)
    sys.stderr.write(r.stderr[-6000:])
    if r.returncode != 0:
        print("measurement failed with exit status %d" % r.returncode)
        return r.returncode or 1
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    with open(OUT, "w") as f:
        f.write(json.dumps(json.loads(line), indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
