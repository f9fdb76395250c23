#!/usr/bin/env python3
"""Cost of the ragged evaluateRange (mtg_evaluate_range_ragged_batch_full) against the
uniform calls it replaces.  1e4 generator trajectories, N = 10, D = 3, K_b uniform over {2, ..., 12},
solved by the ragged solve; dt = 0.01 over the whole trajectory, the one-call form, device-resident
arrays, sample times included.  Times are device events (mtg_kernel_times: a call's first to its last
kernel); a ragged call's host work and its upload of the segment offsets come before its first kernel
and are in none of the figures.

  (a) batch order  one ragged call on the batch as it comes (K_b in random order)
  (b) sorted       one ragged call on the batch sorted by K
  (c) uniform      the sum over K of one mtg_evaluate_range_batch_full call per K-group of the sorted
                   batch (views of the same arrays): the yardstick.  It leaves out the bucketing copies and
                   the re-interleaving of the outputs a caller of the uniform entries needs for (a).

The three are taken in turn inside each of REPS repetitions after a warm-up, outputs rotating over two
buffers; medians and the 10th to 90th percentile are reported, with the bytes written and their rate as
a fraction of the plain-store write ceiling (5.5 TB/s).  The timed outputs are compared
afterwards: (b) equals the concatenated outputs of (c) byte for byte, and (a) its permutation.

Separately, --config2 times the uniform config-2 evaluateRange (K = 10, B = 1e4: scripts/bench_eval.py's
shape) RUNS times, each run a fresh process; with --parent-root DIR the same script is also run on another
checkout of the project (built there), so that the uniform path before and after a change is measured by
the same code.  Every GPU step runs in a child process under a time limit; if one fails nothing is
written.  Writes profiles/evaluate_range_ragged_timing.json.  Needs a HIP device."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "evaluate_range_ragged_timing.json")
N, D, R, B, DT = 10, 3, 4, 10000, 0.01
KS = tuple(range(2, 13))
WARMUP, REPS, RUNS = 5, 30, 5
WRITE_CEILING = 5.5e12
STEP_LIMIT_S = 300


def _stats(np, x):
    return {"median_us": round(float(np.median(x)) * 1e3, 2), "p10_us": round(float(np.percentile(x, 10)) * 1e3, 2),
            "p90_us": round(float(np.percentile(x, 90)) * 1e3, 2), "min_us": round(float(np.min(x)) * 1e3, 2),
            "max_us": round(float(np.max(x)) * 1e3, 2)}


def measure_ragged():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import mav_trajectory_generation_cmake_amd as mtg
    from mav_trajectory_generation_cmake_amd import _native as nat
    from mav_trajectory_generation_cmake_amd.solver import _addr, evaluate_range_capacity

    rng = np.random.default_rng(2024)
    ks = rng.choice(KS, size=B)
    counts = {int(K): int((ks == K).sum()) for K in KS}
    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)
    lib = ctx._lib
    problems = {K: mtg.random_vertices_path_batch(N, D, K, counts[K], seed0=1000 * K) for K in KS}
    sorted_order = [(K, i) for K in KS for i in range(counts[K])]
    batch_order = [sorted_order[j] for j in rng.permutation(B)]
    first = dict(zip(KS, np.concatenate([[0], np.cumsum([counts[K] for K in KS])])))
    to_sorted = np.array([first[K] + i for K, i in batch_order], dtype=np.int64)  # sorted row of every batch row

    def solved(order):
        """(coeffs, times, seg_count) of the ragged device solve of the problems in `order`."""
        v, m, t, seg = mtg.pack_ragged([(problems[K][0][i], problems[K][1][i], problems[K][2][i]) for K, i in order])
        d = [torch.from_numpy(x).to(dev) for x in (v, m, t)]
        sol = ctx.solve_linear_ragged_batch(N, R, d[0], d[1], d[2], seg, status=True)
        torch.cuda.synchronize()
        assert not sol["status"].cpu().numpy().any()
        return sol["coeffs"], d[2], seg

    c_a, t_a, seg_a = solved(batch_order)
    c_b, t_b, seg_b = solved(sorted_order)
    tot_s = int(seg_b.sum())
    # the K-groups of the sorted batch: views of its arrays
    groups, s0 = {}, 0
    for K in KS:
        n = counts[K] * K
        groups[K] = (c_b[s0:s0 + n].view(counts[K], K, D, N), t_b[s0:s0 + n].view(counts[K], K))
        s0 += n
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    F = nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC
    T_END = 1e9

    def ragged_call(c, t, seg, bufs):
        def call(k):
            o, st, cnt, off, tot, cap = bufs[k]
            nat.check(lib.mtg_evaluate_range_ragged_batch_full(ctx.handle, N, D, B, _addr(seg), _addr(c), _addr(t), 0.0,
                                                               T_END, DT, 0, _addr(cnt), _addr(off), _addr(tot), _addr(o),
                                                               _addr(st), cap, F), ctx.handle)
        return call

    def uniform_call(K, bufs):
        c, t = groups[K]

        def call(k):
            o, st, cnt, off, tot, cap = bufs[k]
            nat.check(lib.mtg_evaluate_range_batch_full(ctx.handle, N, D, K, counts[K], _addr(c), _addr(t), 0.0, T_END, DT,
                                                        0, _addr(cnt), _addr(off), _addr(tot), _addr(o), _addr(st), cap,
                                                        F), ctx.handle)
        return call

    def buffers(nb, cap, n=2):
        return [(torch.empty((max(cap, 1), D), dtype=torch.float64, device=dev),
                 torch.empty(max(cap, 1), dtype=torch.float64, device=dev),
                 torch.empty(nb, dtype=torch.int64, device=dev), torch.empty(nb, dtype=torch.int64, device=dev),
                 torch.zeros(1, dtype=torch.int64, device=dev), cap) for _ in range(n)]

    cap = evaluate_range_capacity(t_b, 0.0, T_END, DT, seg_count=seg_b)
    buf_a, buf_b = buffers(B, cap), buffers(B, cap)
    buf_c = {K: buffers(counts[K], evaluate_range_capacity(groups[K][1], 0.0, T_END, DT)) for K in KS}
    call_a, call_b = ragged_call(c_a, t_a, seg_a, buf_a), ragged_call(c_b, t_b, seg_b, buf_b)
    calls_c = [uniform_call(K, buf_c[K]) for K in KS]
    n_c = len(KS)
    ctx.enable_timing(16)
    rows = []
    for rep in range(WARMUP + REPS):
        k = rep % 2
        for call in calls_c:
            call(k)
        call_a(k)
        call_b(k)
        ms = ctx.kernel_times_ms(n_c + 2)  # synchronizes
        assert len(ms) == n_c + 2
        if rep >= WARMUP:
            rows.append((float(ms[n_c]), float(ms[n_c + 1]), float(ms[:n_c].sum())))
    a = np.array(rows)
    torch.cuda.synchronize()

    # the timed outputs: (b) is the concatenation of (c), (a) its permutation
    total = int(buf_b[0][4].item())
    assert total == int(buf_a[0][4].item()) == sum(int(buf_c[K][0][4].item()) for K in KS) <= cap
    same = lambda x, y: bool((x.contiguous().view(torch.int64) == y.contiguous().view(torch.int64)).all())  # noqa: E731
    cat = lambda j, n: torch.cat([buf_c[K][0][j][:n(K)] for K in KS])  # noqa: E731
    nk = lambda K: int(buf_c[K][0][4].item())  # noqa: E731
    assert same(buf_b[0][0][:total], cat(0, nk)) and same(buf_b[0][1][:total], cat(1, nk))
    cnt_b = buf_b[0][2].cpu().numpy()
    assert (cnt_b == cat(2, lambda K: counts[K]).cpu().numpy()).all()
    cnt_a, off_a, off_b = buf_a[0][2].cpu().numpy(), buf_a[0][3].cpu().numpy(), buf_b[0][3].cpu().numpy()
    assert (cnt_a == cnt_b[to_sorted]).all()
    o_a, o_b = buf_a[0][0].cpu().numpy(), buf_b[0][0].cpu().numpy()
    for b in rng.choice(B, size=200, replace=False):  # (every row of 200 trajectories)
        s = to_sorted[b]
        assert (o_a[off_a[b]:off_a[b] + cnt_a[b]].view(np.int64) == o_b[off_b[s]:off_b[s] + cnt_b[s]].view(np.int64)).all()

    written = total * (D + 1) * 8 + 2 * 8 * B + 8
    med = np.median(a, axis=0)

    def rate(us):
        return {"TB_per_s": round(written / (us * 1e-6) / 1e12, 3), "of_write_ceiling": round(written / (us * 1e-6) / WRITE_CEILING, 3)}

    res = {"shape": {"N": N, "D": D, "batch": B, "K": [KS[0], KS[-1]], "counts": counts, "total_segments": tot_s, "dt": DT,
                     "samples": total},
           "reps": REPS, "warmup": WARMUP, "bytes_written": written, "write_ceiling_TB_per_s": WRITE_CEILING / 1e12,
           "offset_bytes_uploaded": 8 * (B + 1),
           "a_ragged_batch_order": dict(_stats(np, a[:, 0]), **rate(med[0] * 1e3)),
           "b_ragged_sorted": dict(_stats(np, a[:, 1]), **rate(med[1] * 1e3)),
           "c_uniform_sum": dict(_stats(np, a[:, 2]), **rate(med[2] * 1e3)),
           "a_over_c": round(float(med[0] / med[2]), 4), "b_over_c": round(float(med[1] / med[2]), 4),
           "outputs_compared": "b == concatenation of c (all bytes); a == permutation of b (counts: all; rows: 200 trajectories)"}
    ctx.close()
    print(json.dumps(res), flush=True)


def measure_config2(root):
    """One run: the uniform config-2 evaluateRange with the package under `root`."""
    import numpy as np
    import torch
    sys.path.insert(0, root)
    import mav_trajectory_generation_cmake_amd as mtg
    from mav_trajectory_generation_cmake_amd import _native as nat
    from mav_trajectory_generation_cmake_amd.solver import _addr, evaluate_range_capacity
    assert os.path.realpath(os.path.dirname(os.path.dirname(mtg.__file__))) == os.path.realpath(root)
    K = 10
    vals, mask, times = mtg.random_vertices_path_batch(N, D, K, B, seed0=0)
    ctx = mtg.Context(0)
    lib = ctx._lib
    dev = torch.device("cuda", 0)
    c_d = torch.from_numpy(ctx.solve_linear_batch(N, R, vals, mask, times)["coeffs"]).to(dev)
    t_d = torch.from_numpy(times).to(dev)
    cap = evaluate_range_capacity(times, 0.0, 1e9, DT)
    bufs = [(torch.empty((cap, D), dtype=torch.float64, device=dev), torch.empty(cap, dtype=torch.float64, device=dev))
            for _ in range(2)]
    cnt, off = (torch.empty(B, dtype=torch.int64, device=dev) for _ in range(2))
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    F = nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC
    ctx.enable_timing(4)
    one, two = [], []
    for rep in range(WARMUP + REPS):
        o, st = bufs[rep % 2]
        nat.check(lib.mtg_evaluate_range_batch_full(ctx.handle, N, D, K, B, _addr(c_d), _addr(t_d), 0.0, 1e9, DT, 0, _addr(cnt),
                                                    _addr(off), _addr(tot), _addr(o), _addr(st), cap, F), ctx.handle)
        # the two-call form's sample call on the counts and offsets the one-call form has just written
        nat.check(lib.mtg_evaluate_range_batch(ctx.handle, N, D, K, B, _addr(c_d), _addr(t_d), 0.0, 1e9, DT, 0, _addr(cnt),
                                               _addr(off), _addr(o), _addr(st), F), ctx.handle)
        ms = ctx.kernel_times_ms(2)
        if rep >= WARMUP:
            one.append(float(ms[0]))
            two.append(float(ms[1]))
    total = int(tot.item())
    ctx.close()
    print(json.dumps({"samples": total, "one_call_median_us": round(float(np.median(one)) * 1e3, 2),
                      "two_call_samples_median_us": round(float(np.median(two)) * 1e3, 2)}), flush=True)


def child(args, what):
    r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__)] + args,
                       capture_output=True, text=True)
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        print("%s failed with exit status %d" % (what, r.returncode))
        sys.exit(r.returncode or 1)  # (nothing further is started on the device)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["ragged", "config2"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--config2", action="store_true", help="also time the uniform config-2 evaluateRange, RUNS runs")
    ap.add_argument("--parent-root", help="another built checkout to time the uniform config-2 evaluateRange on")
    a = ap.parse_args()
    if a.child == "ragged":
        return measure_ragged()
    if a.child == "config2":
        return measure_config2(a.root)
    result = child(["--child", "ragged"], "the ragged measurement")
    if a.config2 or a.parent_root:
        c2 = {"shape": {"N": N, "D": D, "K": 10, "batch": B, "dt": DT}, "runs": RUNS, "reps_per_run": REPS}
        for name, root in (("parent", a.parent_root), ("this", ROOT)):
            if root:
                c2[name] = [child(["--child", "config2", "--root", os.path.abspath(root)], "config 2 on " + name)
                            for _ in range(RUNS)]
        if a.parent_root:
            for key in ("one_call_median_us", "two_call_samples_median_us"):
                p = sorted(r[key] for r in c2["parent"])
                t = sorted(r[key] for r in c2["this"])
                c2[key] = {"parent_min_max": [p[0], p[-1]], "this_median": t[len(t) // 2],
                           "this_median_inside_parent_spread": bool(p[0] <= t[len(t) // 2] <= p[-1])}
        result["uniform_config2"] = c2
    with open(OUT, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
