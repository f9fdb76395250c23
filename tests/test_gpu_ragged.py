"""The ragged solve on the device (mtg_solve_linear_ragged_batch).

The reference of every comparison is the uniform Context.solve_linear_batch on each K-group's packed
arrays with the same flags, and the comparison is assert_array_equal on coeffs, free, n_free, cost and
status: a trajectory's bytes do not depend on the call it is in (include/mtg.h), so the ragged call owes
the uniform call's bytes, gathered or in place."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat
from _ragged_cases import OUTPUTS, assert_matches_groups, order_of, per_k_batches, ragged_of, views_of
from _util import scale_normalised_error

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(free=True, n_free=True, cost=True, status=True)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]


def _uniform_reference(ctx, N, r, batches, **flags):
    """reference[K][name]: the uniform solve of every K-group (device pointers), as numpy."""
    ref = {}
    for K, (v, m, t) in batches.items():
        out = ctx.solve_linear_batch(N, r, *_dev(v, m, t), **ALL, **flags)
        ref[K] = {k: a.cpu().numpy() for k, a in out.items()}
    return ref


def _ragged(ctx, N, r, csr, device, **kw):
    values, mask, times, seg = csr
    if device:
        values, mask, times = _dev(values, mask, times)
    return ctx.solve_linear_ragged_batch(N, r, values, mask, times, seg, **kw)


# column kernel (K = 2, 3, 9), the DL kernel (K = 10) and DLX beyond it; group sizes 1, 10, 11, 64, 65:
# a single trajectory, and the DLX wave's trajectory count and the 64-lane block each +- 1
N10_COUNTS = {2: 10, 3: 65, 9: 11, 10: 64, 11: 65, 12: 10, 13: 11, 21: 64, 50: 1}


@pytest.fixture(scope="module")
def n10(gpu_ctx):
    batches = per_k_batches(10, 3, N10_COUNTS, seed0=77)
    return batches, _uniform_reference(gpu_ctx, 10, 4, batches)


def test_kernels_covered():
    names = {K: mtg.solve_kernel(10, 3, K, 4) for K in N10_COUNTS}
    assert names[2] == names[3] == names[9] == "solve_reg_kernel"
    assert names[10] == "solve_dl_kernel"
    assert all(names[K] == "solve_dlx_kernel" for K in (11, 12, 13, 21, 50))


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_shuffled_n10_equals_uniform(gpu_ctx, n10, pointers):
    batches, ref = n10
    order = order_of(batches, "shuffled", seed=3)
    csr = ragged_of(batches, order)
    plan = mtg.solve_ragged_plan(10, 3, 4, csr[3])
    assert plan["n_groups"] == len(N10_COUNTS) and plan["n_in_place"] == 1      # only the single trajectory
    out = _ragged(gpu_ctx, 10, 4, csr, pointers == "device", **ALL)
    assert set(out) == set(OUTPUTS)
    assert_matches_groups(out, csr[3], 3, order, ref)


def test_sorted_is_in_place_with_guards_and_zero_copy_slices(gpu_ctx, n10):
    batches, ref = n10
    N, D, r, h = 10, 3, 4, 5
    order = order_of(batches, "sorted")
    values, mask, times, seg = ragged_of(batches, order)
    B, totS = len(seg), int(seg.sum())
    totV = totS + B
    assert mtg.solve_ragged_plan(N, D, r, seg)["n_in_place"] == B
    G = 64                      # guard elements before and after every output
    sizes = {"coeffs": totS * D * N, "free": totV * h * D, "n_free": B, "cost": B, "status": B}
    bufs, inner = {}, {}
    for name, n in sizes.items():
        if name in ("n_free", "status"):
            bufs[name] = torch.full((n + 2 * G,), -12345, dtype=torch.int32, device="cuda:0")
        else:
            bufs[name] = torch.full((n + 2 * G,), float("nan"), dtype=torch.float64, device="cuda:0")
        inner[name] = bufs[name][G:G + n]
    inner["coeffs"] = inner["coeffs"].view(totS, D, N)
    out = gpu_ctx.solve_linear_ragged_batch(N, r, *_dev(values, mask, times), seg, **inner)
    assert_matches_groups(out, seg, D, order, ref)
    for name, n in sizes.items():
        g = torch.cat([bufs[name][:G], bufs[name][G + n:]]).cpu().numpy()
        assert (np.isnan(g).all() if g.dtype == np.float64 else (g == -12345).all()), "guard of " + name
        body = inner[name].cpu().numpy()
        if body.dtype == np.int32:      # every element inside was written
            assert (body != -12345).all(), name
        else:
            assert not np.isnan(body).any(), name
    # the zero-copy promise: one group's slice of the ragged coeffs is a uniform array
    K = 11
    vo, so = mtg.ragged_offsets(seg)
    b0 = next(b for b, (k, _) in enumerate(order) if k == K)
    Bk = N10_COUNTS[K]
    c_slice = out["coeffs"][int(so[b0]):int(so[b0]) + Bk * K].view(Bk, K, D, N)
    assert c_slice.data_ptr() == out["coeffs"].data_ptr() + 8 * int(so[b0]) * D * N and c_slice.is_contiguous()
    t_dev = _dev(batches[K][2])[0]
    tq = torch.linspace(0.0, 20.0, 9, dtype=torch.float64, device="cuda:0")
    got = gpu_ctx.evaluate_at_batch(c_slice, t_dev, tq, n_derivatives=2)
    want = gpu_ctx.evaluate_at_batch(_dev(ref[K]["coeffs"])[0], t_dev, tq, n_derivatives=2)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("N,D,r,counts", [(12, 3, 3, {5: 7, 20: 9, 21: 5}), (4, 3, 1, {3: 6, 15: 5}),
                                          (6, 1, 2, {12: 9, 13: 8}), (10, 4, 4, {4: 5, 11: 6, 1: 3})])
def test_other_shapes(gpu_ctx, N, D, r, counts):
    batches = per_k_batches(N, D, counts, seed0=5 * N + D)
    ref = _uniform_reference(gpu_ctx, N, r, batches)
    order = order_of(batches, "shuffled", seed=N)
    csr = ragged_of(batches, order)
    out = _ragged(gpu_ctx, N, r, csr, True, **ALL)
    assert_matches_groups(out, csr[3], D, order, ref)


@pytest.mark.parametrize("kinds", [{10: "vel", 11: "mixed"}, {10: "mixed", 13: "vel"}])
def test_off_pattern_masks_in_gathered_groups(gpu_ctx, kinds):
    """The DL and DLX kernels' general-mask, rest and fallback passes inside gathered groups."""
    counts = {K: 40 for K in kinds}
    counts[5] = 3
    batches = per_k_batches(10, 3, counts, seed0=909, kinds=kinds)
    ref = _uniform_reference(gpu_ctx, 10, 4, batches)
    order = order_of(batches, "shuffled", seed=1)
    csr = ragged_of(batches, order)
    assert mtg.solve_ragged_plan(10, 3, 4, csr[3])["n_in_place"] == 0
    out = _ragged(gpu_ctx, 10, 4, csr, True, **ALL)
    assert_matches_groups(out, csr[3], 3, order, ref)


@pytest.mark.parametrize("how", ["shuffled", "sorted"])
def test_status_bits_gathered_and_in_place(gpu_ctx, how):
    counts = {3: 6, 10: 12, 12: 12}
    batches = {K: tuple(a.copy() for a in v) for K, v in per_k_batches(10, 3, counts, seed0=31).items()}
    for K in (10, 12):
        batches[K][2][2, 1] = -1.0        # MTG_TRAJ_BAD_TIME
        batches[K][2][5, :] = 1e200       # MTG_TRAJ_NOT_SPD
    ref = _uniform_reference(gpu_ctx, 10, 4, batches)
    order = order_of(batches, how, seed=4)
    csr = ragged_of(batches, order)
    in_place = mtg.solve_ragged_plan(10, 3, 4, csr[3])["n_in_place"]
    assert in_place == (len(order) if how == "sorted" else 0)
    out = _ragged(gpu_ctx, 10, 4, csr, True, **ALL)
    assert_matches_groups(out, csr[3], 3, order, ref)
    st = out["status"].cpu().numpy()
    for b, (K, i) in enumerate(order):
        want = {2: nat.MTG_TRAJ_BAD_TIME, 5: nat.MTG_TRAJ_NOT_SPD}.get(i, 0) if K in (10, 12) else 0
        assert (st[b] & want) == want and (want or st[b] == 0), (b, K, i, st[b])


@pytest.mark.parametrize("wanted", [("coeffs",), ("cost", "status")])
def test_nullable_outputs(gpu_ctx, n10, wanted):
    batches, ref = n10
    order = order_of(batches, "shuffled", seed=8)
    csr = ragged_of(batches, order)
    kw = {k: True for k in wanted if k != "coeffs"}
    out = _ragged(gpu_ctx, 10, 4, csr, True, coeffs=None if "coeffs" in wanted else False, **kw)
    assert set(out) == set(wanted)
    assert_matches_groups(out, csr[3], 3, order, ref)


def test_general_flag_passes_through(gpu_ctx, n10):
    batches, _ = n10
    ref = _uniform_reference(gpu_ctx, 10, 4, batches, general=True)
    order = order_of(batches, "shuffled", seed=3)
    csr = ragged_of(batches, order)
    out = _ragged(gpu_ctx, 10, 4, csr, True, general=True, **ALL)
    assert_matches_groups(out, csr[3], 3, order, ref)


def test_split_flag_passes_through(gpu_ctx):
    batches = per_k_batches(10, 3, {3: 5, 10: 6, 12: 4}, seed0=17)
    ref = _uniform_reference(gpu_ctx, 10, 4, batches, split=True)
    order = order_of(batches, "shuffled", seed=2)
    csr = ragged_of(batches, order)
    out = _ragged(gpu_ctx, 10, 4, csr, True, split=True, **ALL)
    assert_matches_groups(out, csr[3], 3, order, ref)


def test_two_async_calls_with_different_plans(gpu_ctx, n10):
    """Back to back on one context, no synchronisation in between: the second call must not overwrite
    the plan records the first call's copy or kernels still read."""
    batches, ref = n10
    calls = []
    for seed in (21, 22):
        order = order_of(batches, "shuffled", seed=seed)
        if seed == 22:
            order = order[:150]      # another batch size too: other offsets, other group sizes
        values, mask, times, seg = ragged_of(batches, order)
        calls.append((order, seg, _dev(values, mask, times)))
    sub = {K: sum(1 for k, _ in calls[1][0] if k == K) for K in batches}
    outs = [gpu_ctx.solve_linear_ragged_batch(10, 4, *dev, seg, asynchronous=True, **ALL) for _, seg, dev in calls]
    torch.cuda.synchronize()
    assert_matches_groups(outs[0], calls[0][1], 3, calls[0][0], ref)
    # the second batch holds a part of every group: the uniform reference of exactly those members
    order2 = calls[1][0]
    part = {K: (np.stack([batches[K][0][i] for k, i in order2 if k == K]),
                np.stack([batches[K][1][i] for k, i in order2 if k == K]),
                np.stack([batches[K][2][i] for k, i in order2 if k == K])) for K in batches if sub[K]}
    ref2 = _uniform_reference(gpu_ctx, 10, 4, part)
    seen = {K: 0 for K in part}
    renum = []
    for K, _ in order2:
        renum.append((K, seen[K]))
        seen[K] += 1
    assert_matches_groups(outs[1], calls[1][1], 3, renum, ref2)


def test_device_result_against_host_ragged(gpu_ctx, n10):
    """An independent check: the library's host path on the same CSR arrays, at the figures
    test_host_path_matches_gpu (tests/test_gpu_parity.py) holds the uniform paths to."""
    batches, _ = n10
    order = order_of(batches, "shuffled", seed=3)
    csr = ragged_of(batches, order)
    g = _ragged(gpu_ctx, 10, 4, csr, True, **ALL)
    h = mtg.host_solve_linear_ragged_batch(10, 4, *csr, free=True, n_free=True, cost=True, status=True, threads=4)
    np.testing.assert_array_equal(h["status"], g["status"].cpu().numpy())
    np.testing.assert_array_equal(h["n_free"], g["n_free"].cpu().numpy())
    np.testing.assert_allclose(h["cost"], g["cost"].cpu().numpy(), rtol=1e-9)
    gc = mtg.split_ragged(g["coeffs"].cpu().numpy(), csr[3], "coeffs")
    hc = mtg.split_ragged(h["coeffs"], csr[3], "coeffs")
    tt = mtg.split_ragged(csr[2], csr[3], "times")
    worst = max(scale_normalised_error(hc[b][None], gc[b][None], tt[b][None]) for b in range(len(order)))
    assert worst <= 1e-9, worst


def test_cpp_solve_ragged_on_device(tmp_path, gpu_ctx):
    """tests/cpp/test_ragged.cpp: solveRagged from vertex lists of 3, 11 and 12 vertices against three
    PolynomialOptimization<10> drop-in solves.  Built with g++ against the library in the tree."""
    cxx = shutil.which("g++") or "g++"
    exe = str(tmp_path / "test_ragged")
    libdir = os.path.dirname(nat.LIB_PATH)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-DMTG_CPP_THROW=1", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_ragged.cpp"),
                    "-o", exe, "-L", libdir, "-lmav_trajectory_generation", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
