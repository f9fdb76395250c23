#!/usr/bin/env python3
"""Cost of the ragged solve (mtg_solve_linear_ragged_batch) against the uniform calls it
replaces.  1e4 trajectories, N = 10, D = 3, r = 4, K uniform over {5, ..., 15}, device-resident arrays,
coefficients only; times are device events (mtg_kernel_times: a call's first to its last kernel).

  (a) uniform   the sum over K of one mtg_solve_linear_batch per K-group on packed arrays (the baseline)
  (b) sorted    one ragged call on the batch sorted by K: every group in place, the same kernels on the
                same bytes as (a), plus the gaps between its launches
  (c) shuffled  one ragged call on the shuffled batch: every group gathered, i.e. (b) plus the gather and
                scatter kernels (one read and one write of every input and output byte)

The three are taken in turn inside every repetition, after a warm-up of every shape, and the timed calls'
coefficients are compared with the uniform calls' afterwards.  The GPU work runs in a child process under
a time limit; if it fails or times out nothing is written.  Writes profiles/ragged_timing.json.  Needs a
HIP device."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "ragged_timing.json")
N, D, R, B = 10, 3, 4, 10000
KS = tuple(range(5, 16))
WARMUP, REPS = 10, 60
STEP_LIMIT_S = 240


def measure():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import mav_trajectory_generation_cmake_amd as mtg

    rng = np.random.default_rng(2024)
    ks = rng.choice(KS, size=B)
    counts = {int(K): int((ks == K).sum()) for K in KS}
    batches = {K: mtg.random_vertices_path_batch(N, D, K, counts[K], seed0=1000 * K) for K in KS}
    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # (a): one bound call per K-group
    uniform, ref, keep = [], {}, []
    for K in KS:
        v, m, t = (to_dev(a) for a in batches[K])
        c = torch.zeros((counts[K], K, D, N), dtype=torch.float64, device=dev)
        uniform.append(ctx.solve_call(N, R, v, m, t, c))
        keep.append((v, m, t))      # (solve_call binds addresses only)
        ref[K] = c

    def ragged_case(order):
        values, mask, times, seg = mtg.pack_ragged([(batches[K][0][i], batches[K][1][i], batches[K][2][i])
                                                    for K, i in order])
        arrs = [to_dev(a) for a in (values, mask, times)]
        coeffs = torch.zeros((int(seg.sum()), D, N), dtype=torch.float64, device=dev)
        plan = mtg.solve_ragged_plan(N, D, R, seg)

        def call():
            ctx.solve_linear_ragged_batch(N, R, *arrs, seg, coeffs=coeffs, asynchronous=True)
        return call, coeffs, seg, plan

    sorted_order = [(K, i) for K in KS for i in range(counts[K])]
    shuffled = [sorted_order[j] for j in rng.permutation(B)]
    call_b, coeffs_b, seg_b, plan_b = ragged_case(sorted_order)
    call_c, coeffs_c, seg_c, plan_c = ragged_case(shuffled)
    assert plan_b["n_in_place"] == B and plan_c["n_in_place"] == 0, (plan_b, plan_c)

    ctx.enable_timing(16)
    n_a = len(uniform)
    rows = []
    for rep in range(WARMUP + REPS):
        for step in uniform:
            step()
        call_b()
        call_c()
        ms = ctx.kernel_times_ms(n_a + 2)      # synchronizes
        assert len(ms) == n_a + 2
        if rep >= WARMUP:
            rows.append((float(ms[:n_a].sum()), float(ms[n_a]), float(ms[n_a + 1])) + tuple(float(x) for x in ms[:n_a]))
    torch.cuda.synchronize()
    # the timed calls computed what the uniform calls computed (a NaN, which a trajectory of the bench
    # generator with a near-zero segment can give, equals a NaN)
    def same(x, y):
        x, y = x.reshape(y.shape), y
        ok = (x == y) | (x.isnan() & y.isnan())
        if not bool(ok.all()):
            bad = torch.nonzero(~ok)
            print("mismatch: %d elements, first at %s: %r vs %r" % (bad.shape[0], bad[0].tolist(), x[tuple(bad[0])].item(),
                                                                     y[tuple(bad[0])].item()), file=sys.stderr)
        return bool(ok.all())

    so = np.concatenate([[0], np.cumsum(seg_b)])
    b0 = 0
    for K in KS:
        got = coeffs_b[int(so[b0]):int(so[b0 + counts[K]])].view(counts[K], K, D, N)
        assert same(got, ref[K]), K
        b0 += counts[K]
    pos = {key: b for b, key in enumerate(shuffled)}
    so_c = np.concatenate([[0], np.cumsum(seg_c)])
    for K in KS:
        for i in (0, counts[K] - 1):
            b = pos[(K, i)]
            assert same(coeffs_c[int(so_c[b]):int(so_c[b + 1])], ref[K][i]), (K, i)
    ctx.close()

    a = np.array(rows)
    tot_s = int(seg_b.sum())
    tot_v = tot_s + B
    in_bytes = 8 * tot_v * (N // 2) * D + tot_v + 8 * tot_s
    out_bytes = 8 * tot_s * D * N

    def stats(x):
        return {"median_us": round(float(np.median(x)) * 1e3, 2), "p10_us": round(float(np.percentile(x, 10)) * 1e3, 2),
                "p90_us": round(float(np.percentile(x, 90)) * 1e3, 2)}

    res = {"shape": {"N": N, "D": D, "r": R, "batch": B, "K": [KS[0], KS[-1]], "counts": counts,
                     "total_segments": tot_s, "outputs": "coeffs"},
           "reps": REPS, "warmup": WARMUP,
           "a_uniform_sum": stats(a[:, 0]), "b_ragged_sorted": stats(a[:, 1]), "c_ragged_shuffled": stats(a[:, 2]),
           "a_per_K_median_us": {str(K): round(float(np.median(a[:, 3 + i])) * 1e3, 2) for i, K in enumerate(KS)},
           "b_over_a": round(float(np.median(a[:, 1]) / np.median(a[:, 0])), 4),
           "c_over_b": round(float(np.median(a[:, 2]) / np.median(a[:, 1])), 4),
           "gather_scatter": {"bytes_read_and_written": 2 * (in_bytes + out_bytes),
                              "c_minus_b_us": round(float(np.median(a[:, 2] - a[:, 1])) * 1e3, 2)}}
    gs = res["gather_scatter"]
    gs["effective_TB_per_s"] = round(gs["bytes_read_and_written"] / max(gs["c_minus_b_us"], 1e-9) / 1e6, 3)
    print(json.dumps(res), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        measure()
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child"],
                       capture_output=True, text=True)
    sys.stderr.write(r.stderr[-4000:])
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
