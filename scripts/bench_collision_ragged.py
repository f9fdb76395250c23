#!/usr/bin/env python3
"""Cost of the ragged vertex derivatives and collision cost (mtg_vertex_derivatives_ragged_batch,
mtg_collision_cost_ragged_batch) against the uniform calls they replace.  The shape of
scripts/bench_evaluate_ragged.py: N = 10, D = 3, solved coefficients, device-resident arrays; times are
device events (mtg_kernel_times: a call's one kernel).  A ragged call's host work and its upload of the
segment offsets come before its kernel and are in none of the figures.

  (a) uniform   the sum over K of one uniform call per K-group on packed arrays: the baseline.  It leaves
                out the bucketing copies a caller of the uniform entries needs for an unsorted batch.
  (b) sorted    one ragged call on the batch sorted by K
  (c) shuffled  one ragged call on the shuffled batch

for vertex_derivatives alone, collision_cost (with the gradient) alone, and the chain of the two, on two
mixes: "mix-5-15", the K mix of DESIGN.md 3.14 (1e4 trajectories, K uniform over {5, ..., 15}), and
"mix-5-15-and-50", the same with a group of 100 trajectories of K = 50 added -- one launch has one LDS
size, so there every short trajectory of the ragged collision call runs at the K = 50 occupancy.

Every case is warmed up, then (a), (b), (c) are taken in turn inside each of REPS repetitions; the median
and the 10th to 90th percentile are reported, and the timed calls' outputs are compared with the uniform
calls' afterwards.  The GPU work runs in a child process under a time limit; if it fails or times out
nothing is written.  Writes profiles/collision_ragged_timing.json.  Needs a HIP device."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "collision_ragged_timing.json")
N, D, R, B = 10, 3, 4, 10000
KS = tuple(range(5, 16))
K_LONG, B_LONG = 50, 100
WARMUP, REPS = 5, 30
STEP_LIMIT_S = 420


def sphere_field(n=64, origin=-8.0, resolution=0.25, seed=7, spheres=12):
    """Union of spheres min_i(|p - c_i| - r_i) at the cell centres, float32."""
    import numpy as np
    rng = np.random.default_rng(seed)
    centres = rng.uniform(origin + 2.0, origin + n * resolution - 2.0, size=(spheres, 3))
    radii = rng.uniform(0.5, 1.5, size=spheres)
    ax = origin + (np.arange(n) + 0.5) * resolution
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    d = np.full((n, n, n), np.inf)
    for c, r in zip(centres, radii):
        d = np.minimum(d, np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r)
    return d.astype(np.float32), (origin,) * 3, resolution


def measure():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import mav_trajectory_generation_cmake_amd as mtg
    from mav_trajectory_generation_cmake_amd import _native as nat
    from mav_trajectory_generation_cmake_amd.solver import _addr

    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)
    lib = ctx._lib
    h = N // 2
    field, origin, res = sphere_field()
    grid = mtg.SdfGrid(torch.from_numpy(field).to(dev), origin, res, 0.75)
    prm = mtg.CollisionParams(0.1, 0.2, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True)
    gn, keep = grid.native()
    pn = prm.native()
    F = nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def stats(x):
        return {"median_us": round(float(np.median(x)) * 1e3, 2), "p10_us": round(float(np.percentile(x, 10)) * 1e3, 2),
                "p90_us": round(float(np.percentile(x, 90)) * 1e3, 2)}

    def same_bits(x, y):
        x, y = x.contiguous().view(torch.uint8).reshape(-1), y.contiguous().view(torch.uint8).reshape(-1)
        return x.shape == y.shape and bool((x == y).all())

    def run_mix(name, counts, seed):
        rng = np.random.default_rng(seed)
        ks = sorted(counts)
        nB = sum(counts.values())
        coeffs, times, masks, vv = {}, {}, {}, {}
        for K in ks:
            v, m, t = mtg.random_vertices_path_batch(N, D, K, counts[K], seed0=1000 * K)
            coeffs[K], times[K], masks[K] = ctx.solve_linear_batch(N, R, v, m, t)["coeffs"], t, m
            vv[K] = ctx.vertex_derivatives_batch(coeffs[K], t)
        sorted_order = [(K, i) for K in ks for i in range(counts[K])]
        shuffled = [sorted_order[j] for j in rng.permutation(nB)]
        g = {K: dict(c=to_dev(coeffs[K]), t=to_dev(times[K]), m=to_dev(masks[K]), x=to_dev(vv[K])) for K in ks}

        def csr(order):
            return dict(c=to_dev(np.concatenate([coeffs[K][i] for K, i in order])),
                        t=to_dev(np.concatenate([times[K][i] for K, i in order])),
                        m=to_dev(np.concatenate([masks[K][i] for K, i in order])),
                        x=to_dev(np.concatenate([vv[K][i] for K, i in order])),
                        seg=np.array([K for K, _ in order], dtype=np.int32))

        cs = {"b": csr(sorted_order), "c": csr(shuffled)}
        tot_s = int(cs["b"]["seg"].sum())
        tot_v = tot_s + nB
        # outputs: the uniform groups' and the two ragged calls'
        o_a = {K: dict(x=torch.empty((counts[K], K + 1, h, D), dtype=torch.float64, device=dev),
                       cost=torch.empty(counts[K], dtype=torch.float64, device=dev),
                       grad=torch.empty((counts[K], D, (K + 1) * h), dtype=torch.float64, device=dev),
                       coll=torch.empty(counts[K], dtype=torch.uint8, device=dev),
                       nev=torch.empty(counts[K], dtype=torch.int32, device=dev),
                       st=torch.empty(counts[K], dtype=torch.int32, device=dev)) for K in ks}
        o_r = {w: dict(x=torch.empty((tot_v, h, D), dtype=torch.float64, device=dev),
                       cost=torch.empty(nB, dtype=torch.float64, device=dev),
                       grad=torch.empty(tot_v * h * D, dtype=torch.float64, device=dev),
                       coll=torch.empty(nB, dtype=torch.uint8, device=dev),
                       nev=torch.empty(nB, dtype=torch.int32, device=dev),
                       st=torch.empty(nB, dtype=torch.int32, device=dev)) for w in ("b", "c")}
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        ctx.enable_timing(64)

        def vd_uniform(K, x_in=None):
            nat.check(lib.mtg_vertex_derivatives_batch(ctx.handle, N, D, K, counts[K], _addr(g[K]["c"]), _addr(g[K]["t"]),
                                                       _addr(o_a[K]["x"]), F), ctx.handle)

        def cc_uniform(K, chained=False):
            o = o_a[K]
            x = o["x"] if chained else g[K]["x"]
            nat.check(lib.mtg_collision_cost_batch(ctx.handle, N, D, K, counts[K], _addr(x), _addr(g[K]["m"]),
                                                   _addr(g[K]["t"]), ctypes.byref(gn), ctypes.byref(pn), _addr(o["cost"]),
                                                   _addr(o["grad"]), _addr(o["coll"]), _addr(o["nev"]), _addr(o["st"]), F),
                      ctx.handle)

        def vd_ragged(w):
            a, o = cs[w], o_r[w]
            nat.check(lib.mtg_vertex_derivatives_ragged_batch(ctx.handle, N, D, nB, _addr(a["seg"]), _addr(a["c"]),
                                                              _addr(a["t"]), _addr(o["x"]), F), ctx.handle)

        def cc_ragged(w, chained=False):
            a, o = cs[w], o_r[w]
            x = o["x"] if chained else a["x"]
            nat.check(lib.mtg_collision_cost_ragged_batch(ctx.handle, N, D, nB, _addr(a["seg"]), _addr(x), _addr(a["m"]),
                                                          _addr(a["t"]), ctypes.byref(gn), ctypes.byref(pn),
                                                          _addr(o["cost"]), _addr(o["grad"]), _addr(o["coll"]),
                                                          _addr(o["nev"]), _addr(o["st"]), F), ctx.handle)

        entries = {
            "vertex_derivatives": (1, lambda K: vd_uniform(K), lambda w: vd_ragged(w)),
            "collision_cost": (1, lambda K: cc_uniform(K), lambda w: cc_ragged(w)),
            "chain": (2, lambda K: (vd_uniform(K), cc_uniform(K, True)), lambda w: (vd_ragged(w), cc_ragged(w, True))),
        }
        out = {"counts": {str(K): counts[K] for K in ks}, "batch": nB, "total_segments": tot_s, "offset_bytes": 8 * (nB + 1),
               "lds_bytes_ragged_collision": 8 * (max(ks) * 3 * N + max(ks) + (max(ks) + 1) * h * 3 + 3 * 65 + 64),
               "entries": {}}
        for ename, (per, uni, rag) in entries.items():
            rows = []
            n_a = per * len(ks)
            for rep in range(WARMUP + REPS):
                for K in ks:
                    uni(K)
                rag("b")
                rag("c")
                ms = ctx.kernel_times_ms(n_a + 2 * per)  # synchronizes
                assert len(ms) == n_a + 2 * per
                if rep >= WARMUP:
                    rows.append((float(ms[:n_a].sum()), float(ms[n_a:n_a + per].sum()), float(ms[n_a + per:].sum())))
            a = np.array(rows)
            r = {"a_uniform_sum": stats(a[:, 0]), "b_ragged_sorted": stats(a[:, 1]), "c_ragged_shuffled": stats(a[:, 2]),
                 "b_over_a": round(float(np.median(a[:, 1]) / np.median(a[:, 0])), 4),
                 "c_over_a": round(float(np.median(a[:, 2]) / np.median(a[:, 0])), 4), "uniform_calls": len(ks)}
            torch.cuda.synchronize()
            # the timed calls' outputs against the uniform calls' (sorted batch: the groups in a row)
            if ename != "collision_cost":
                assert same_bits(o_r["b"]["x"], torch.cat([o_a[K]["x"].reshape(-1, h, D) for K in ks])), (name, ename, "x")
            if ename != "vertex_derivatives":
                for key in ("cost", "coll", "nev", "st"):
                    assert same_bits(o_r["b"][key], torch.cat([o_a[K][key] for K in ks])), (name, ename, key)
                assert same_bits(o_r["b"]["grad"], torch.cat([o_a[K]["grad"].reshape(-1) for K in ks])), (name, ename, "grad")
                first = dict(zip(ks, np.concatenate([[0], np.cumsum([counts[K] for K in ks])])))
                to_sorted = to_dev(np.array([first[K] + i for K, i in shuffled], dtype=np.int64))
                assert same_bits(o_r["c"]["cost"], o_r["b"]["cost"][to_sorted]), (name, ename, "shuffled cost")
                r["samples_evaluated"] = int(o_r["b"]["nev"].sum().item())
            out["entries"][ename] = r
            print(json.dumps({name: {ename: r}}), file=sys.stderr, flush=True)
        return out

    rng = np.random.default_rng(2024)
    ks = rng.choice(KS, size=B)
    counts = {int(K): int((ks == K).sum()) for K in KS}
    result = {"shape": {"N": N, "D": D}, "reps": REPS, "warmup": WARMUP, "mixes": {}}
    result["mixes"]["mix-5-15"] = run_mix("mix-5-15", counts, 1)
    result["mixes"]["mix-5-15-and-50"] = run_mix("mix-5-15-and-50", {**counts, K_LONG: B_LONG}, 2)
    del keep
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
