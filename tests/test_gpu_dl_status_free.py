"""The DL solve kernel's two instantiations (csrc/mtg_solve_dl.inc): a launch that asks for no status,
cost or n_free runs without the checks that produce them (ST = false); one that asks runs with them
(ST = true).  Both do the same f64 operations on the solution's path, so their coefficients are equal
bit for bit -- on every pass, both output alignments, a partial last wave, one full wave and one
trajectory over -- and both read their arguments through the hot kernarg header (DlHot), the time
sweep and the cold passes through the full arguments behind it."""
import functools

import numpy as np
import pytest

from _util import scale_normalised_error

pytestmark = pytest.mark.gpu

SHAPES = [(10, 10, 4), (12, 20, 3)]          # (N, K, r): the chain lengths the kernel is built for
BATCHES = (1, 9, 10, 11, 23)                 # D = 3: a partial wave, 10 = one full wave, one trajectory over, ...
BMAX = max(BATCHES)
HOST_TOL = 1e-9                              # tests/test_gpu_parity.py test_host_path_matches_gpu


@functools.lru_cache(maxsize=None)
def _inputs(N, K, D, gen):
    """BMAX generator-pattern trajectories (read-only; the smaller batches are their leading ones)."""
    import mav_trajectory_generation_cmake_amd as mtg
    if gen == "path":
        out = mtg.random_vertices_path_batch(N, D, K, BMAX, seed0=900 + N + D)
    else:
        out = mtg.random_vertices_batch(N, D, K, BMAX, [-50.0] * D, [50.0] * D, seed0=700 + N + D)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _host(N, K, r, D, gen):
    import mav_trajectory_generation_cmake_amd as mtg
    vals, mask, times = _inputs(N, K, D, gen)
    c = mtg.host_solve_linear_batch(N, r, vals, mask, times)["coeffs"]
    c.setflags(write=False)
    return c


# The one input on which the host reference is itself further than HOST_TOL from the 60-digit truth
# (tests/golden/make_golden.py truth_solve, worked out on the host): trajectory 16 of the N = 10, 1-D
# createRandomVertices batch, segment times 0.97 .. 51.7.  The best FP64 solve is 8.7e-10 from truth
# there and the host path 1.96e-9, so an exact solver would stand 1.96e-9 from the host: that
# trajectory alone is held to the host reference's own error, 2e-9, instead of HOST_TOL (the kernel
# measured 1.28e-9 from the host there, before and after it had a status-free instantiation).
ILL_CONDITIONED = {(10, 1, "vertices", 16): 2e-9}


def _check_vs_host(N, D, gen, times, host, coeffs):
    """Every trajectory within HOST_TOL of the host path's (ILL_CONDITIONED: the one named exception)."""
    errs = np.array([scale_normalised_error(host[b:b + 1], coeffs[b:b + 1], times[b:b + 1]) for b in range(len(coeffs))])
    for b, e in enumerate(errs):
        tol = ILL_CONDITIONED.get((N, D, gen, b), HOST_TOL)
        assert e <= tol, (N, D, gen, b, e, tol)
    return float(errs.max())


def _dl(N, D, K, r, B):
    from mav_trajectory_generation_cmake_amd import _native as nat
    assert nat.solve_kernel(N, D, K, r, B=B) == "solve_dl_kernel"


@pytest.mark.parametrize("gen", ["path", "vertices"])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("N,K,r", SHAPES)
def test_status_free_equals_status_and_host(gpu_ctx, N, K, r, D, gen):
    vals, mask, times = _inputs(N, K, D, gen)
    host = _host(N, K, r, D, gen)
    _dl(N, D, K, r, BMAX)
    whole = gpu_ctx.solve_linear_batch(N, r, vals, mask, times)["coeffs"]
    err = _check_vs_host(N, D, gen, times, host, whole)
    print("N=%d D=%d %s: vs host %.3e" % (N, D, gen, err))
    for B in BATCHES:
        v, m, t = vals[:B], mask[:B], times[:B]
        plain = gpu_ctx.solve_linear_batch(N, r, v, m, t)                      # ST = false
        withst = gpu_ctx.solve_linear_batch(N, r, v, m, t, status=True)       # ST = true
        assert "status" not in plain and (withst["status"] == 0).all()
        np.testing.assert_array_equal(plain["coeffs"], withst["coeffs"], err_msg="B=%d" % B)
        # a trajectory's bits do not depend on its batch: every batch size equals what was checked
        # against the host above
        np.testing.assert_array_equal(plain["coeffs"], whole[:B], err_msg="B=%d" % B)
        # free values alone need no status either (ST = false with an optional output asked for)
        fr = gpu_ctx.solve_linear_batch(N, r, v, m, t, free=True)
        full = gpu_ctx.solve_linear_batch(N, r, v, m, t, free=True, n_free=True, cost=True, status=True)
        np.testing.assert_array_equal(fr["coeffs"], plain["coeffs"])
        np.testing.assert_array_equal(full["coeffs"], plain["coeffs"])
        np.testing.assert_array_equal(fr["free"], full["free"])


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("N,K,r", SHAPES)
def test_output_only_8_byte_aligned(gpu_ctx, N, K, r, D):
    """AL16 = 0 (8-byte pieces) in both instantiations, on device arrays."""
    import torch
    vals, mask, times = _inputs(N, K, D, "path")
    host = _host(N, K, r, D, "path")
    dev = torch.device("cuda:0")
    for B in BATCHES:
        dv, dm, dt = (torch.from_numpy(np.array(x[:B])).to(dev) for x in (vals, mask, times))
        shape = (B, K, D, N)
        c16 = torch.zeros(shape, dtype=torch.float64, device=dev)
        gpu_ctx.solve_linear_batch(N, r, dv, dm, dt, coeffs=c16)
        outs = []
        for st in (False, True):
            buf = torch.zeros(B * K * D * N + 1, dtype=torch.float64, device=dev)
            c8 = buf[1:].view(shape)
            assert c8.data_ptr() % 16 == 8
            status = torch.full((B,), -1, dtype=torch.int32, device=dev) if st else None
            gpu_ctx.solve_linear_batch(N, r, dv, dm, dt, coeffs=c8, status=status)
            torch.cuda.synchronize()
            if st:
                assert (status.cpu().numpy() == 0).all()
            outs.append(c8.cpu().numpy())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(outs[0], outs[1], err_msg="B=%d" % B)
        np.testing.assert_array_equal(outs[0], c16.cpu().numpy(), err_msg="B=%d" % B)
        _check_vs_host(N, D, "path", times[:B], host[:B], outs[0])


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("N,K,r", SHAPES)
def test_time_sweep_three_candidates(gpu_ctx, N, K, r, D):
    """n_cand = 3 with scales: pair p solves trajectory p / 3 with its times scaled (the sweep's
    divisions, read from the arguments behind the header) -- the host path's costs at the scaled
    times, and the costs of separate GPU solves there.  (The sweep always asks for the cost, so it
    runs the instantiation with the checks: the C ABI has no status-free sweep.)"""
    import mav_trajectory_generation_cmake_amd as mtg
    vals, mask, times = _inputs(N, K, D, "path")
    scales = np.array([0.7, 1.0, 1.9])
    # an independent reference: the host path's cost at the scaled times (rtol: test_host_path_matches_gpu)
    host = np.stack([mtg.host_solve_linear_batch(N, r, vals, mask, times * s, cost=True)["cost"] for s in scales], axis=1)
    J = gpu_ctx.time_sweep_batch(N, r, vals, mask, times, scales)
    print("N=%d D=%d sweep vs host cost: max rel %.3e" % (N, D, np.max(np.abs(J - host) / np.abs(host))))
    np.testing.assert_allclose(J, host, rtol=1e-9, atol=0)
    for B in BATCHES:
        v, m, t = vals[:B], mask[:B], times[:B]
        _dl(N, D, K, r, 3 * B)
        J = gpu_ctx.time_sweep_batch(N, r, v, m, t, scales)
        assert J.shape == (B, 3)
        for ci, s in enumerate(scales):
            ref = gpu_ctx.solve_linear_batch(N, r, v, m, t * s, cost=True)["cost"]
            np.testing.assert_allclose(J[:, ci], ref, rtol=1e-9, atol=0, err_msg="B=%d c=%d" % (B, ci))


@pytest.mark.parametrize("N,K,r", SHAPES)
def test_mixed_batch_cold_passes(gpu_ctx, N, K, r):
    """3 of 11 trajectories off the pattern -- ends fixed to ACCELERATION only (the ends pass), a fixed
    interior velocity (the general-mask pass), a free interior position (the fallback): the cold
    passes find their arguments, with and without the status."""
    import mav_trajectory_generation_cmake_amd as mtg
    D, B = 3, 11
    vals, mask, times = (x[:B].copy() for x in _inputs(N, K, D, "path"))
    rng = np.random.default_rng(5)
    mask[2, 0] = mask[2, K] = 0b111
    mask[5, 3] |= 2
    vals[5, 3, 1, :] = rng.normal(size=D)
    mask[8, K // 2] &= 0xFE
    host = mtg.host_solve_linear_batch(N, r, vals, mask, times, status=True, n_free=True)
    plain = gpu_ctx.solve_linear_batch(N, r, vals, mask, times)
    withst = gpu_ctx.solve_linear_batch(N, r, vals, mask, times, status=True, n_free=True)
    np.testing.assert_array_equal(plain["coeffs"], withst["coeffs"])
    np.testing.assert_array_equal(withst["status"], host["status"])
    np.testing.assert_array_equal(withst["n_free"], host["n_free"])
    assert (withst["status"] == 0).all()
    for b in range(B):
        err = scale_normalised_error(host["coeffs"][b:b + 1], plain["coeffs"][b:b + 1], times[b:b + 1])
        assert err <= HOST_TOL, (b, err)


# include/mtg.h: MTG_TRAJ_BAD_TIME 1, MTG_TRAJ_NOT_SPD 2.  What the kernel reported before it had a
# status-free instantiation, recorded here (not recomputed): a zero, a negative and a NaN segment time
# are BAD_TIME, and the factorisation they break is NOT_SPD as well; 1e-200 is a valid time whose
# system leaves the double range, NOT_SPD alone.
BAD_TIME, NOT_SPD = 1, 2
RECORDED_STATUS = {0: BAD_TIME | NOT_SPD, 1: BAD_TIME | NOT_SPD, 2: BAD_TIME | NOT_SPD, 3: NOT_SPD}


@pytest.mark.parametrize("N,K,r", SHAPES)
def test_statuses_unchanged(gpu_ctx, N, K, r):
    D, B = 3, 11
    vals, mask, times = (x[:B].copy() for x in _inputs(N, K, D, "path"))
    times[0, 2] = 0.0
    times[1, 3] = -1.0
    times[2, 1] = np.nan
    times[3, 4] = 1e-200
    st = gpu_ctx.solve_linear_batch(N, r, vals, mask, times, status=True)["status"]
    print("N=%d statuses %s" % (N, st.tolist()))
    want = np.zeros(B, dtype=st.dtype)
    for b, s in RECORDED_STATUS.items():
        want[b] = s
    np.testing.assert_array_equal(st, want)
    # the same call without the status still solves the good trajectories to the same bits
    good = gpu_ctx.solve_linear_batch(N, r, vals[4:], mask[4:], times[4:], status=True)["coeffs"]
    plain = gpu_ctx.solve_linear_batch(N, r, vals, mask, times)["coeffs"]
    np.testing.assert_array_equal(plain[4:], good)
