"""Soft-constraint cost and gradient of the magnitude limits on the GPU
(mtg_soft_constraint_cost_batch): the kernel -- which searches only the one or two segments a
perturbation touches -- against the independent FP64 model and against the host path (the literal
full re-evaluation) on the shared cases of tests/_soft_constraint_model.py, plus the bit-level
properties of the call."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat
from mav_trajectory_generation_cmake_amd.solver import EXTREMUM_DTYPE

import _soft_constraint_model as M
from test_soft_constraint_host import invalid_calls

pytestmark = pytest.mark.gpu


def _device(ctx, name, grad=True):
    N, x, mask, times, prm = M.case(name)
    return ctx.soft_constraint_cost_batch(N, x, times, prm.native(), mask=mask, grad=grad)


def _host(name):
    N, x, mask, times, prm = M.case(name)
    return mtg.host_soft_constraint_cost_batch(N, x, times, prm.native(), mask=mask, grad=True, threads=8)


def _same_bits(a, b):
    for key in ("cost", "grad", "maxima", "status"):
        if a[key] is None or b[key] is None:
            continue
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("name", M.ALL_CASES)
def test_device_matches_model_and_host(gpu_ctx, name):
    dev = _device(gpu_ctx, name)
    M.compare("device vs model", dev, name)
    M.compare("device vs host", dev, name, other=_host(name))


def test_locality_is_exact(gpu_ctx):
    """A free derivative of a vertex that is not an end of the dominating segment: exactly 0.0."""
    N, x, mask, times, prm = M.case("locality")
    out = _device(gpu_ctx, "locality")
    h = N // 2
    for b, m in enumerate(M.model("locality")):
        s = m["maxima"][0][2]
        slots = [(v, k) for v in range(x.shape[1]) for k in range(h) if not (int(mask[b, v]) >> k) & 1]
        far = [n for n, (v, k) in enumerate(slots) if v not in (s, s + 1)]
        assert len(far) >= 24 and (out["grad"][b][:, far] == 0.0).all()


def test_saturation_is_exact(gpu_ctx):
    N, x, mask, times, prm = M.case("saturated")
    out = _device(gpu_ctx, "saturated")
    assert (out["cost"] == len(prm.constraints) * 1e12).all()
    assert (out["grad"] == 0.0).all()


@pytest.mark.parametrize("name", ["config2", "d1_n8"])
def test_gradient_off_leaves_the_cost_bits(gpu_ctx, name):
    a, b = _device(gpu_ctx, name), _device(gpu_ctx, name, grad=False)
    assert b["grad"] is None
    _same_bits(a, b)


def test_bits_do_not_depend_on_batch_position_or_call(gpu_ctx):
    N, x, mask, times, prm = M.case("config2")
    full = _device(gpu_ctx, "config2")
    perm = np.random.default_rng(5).permutation(x.shape[0])
    shuffled = gpu_ctx.soft_constraint_cost_batch(N, x[perm], times[perm], prm.native(), mask=mask[perm], grad=True)
    for key in ("cost", "grad", "maxima", "status"):
        assert shuffled[key].tobytes() == full[key][perm].tobytes(), key
    for b in (0, 33, 66):
        one = gpu_ctx.soft_constraint_cost_batch(N, x[b:b + 1], times[b:b + 1], prm.native(), mask=mask[b:b + 1],
                                                 grad=True)
        for key in ("cost", "grad", "maxima", "status"):
            assert one[key].tobytes() == full[key][b:b + 1].tobytes(), (key, b)


def test_device_pointers_and_asynchronous_call(gpu_ctx):
    import torch
    N, x, mask, times, prm = M.case("config2")
    full = _device(gpu_ctx, "config2")
    dx, dm, dt = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, mask, times))
    for asynchronous in (False, True):
        out = gpu_ctx.soft_constraint_cost_batch(N, dx, dt, prm.native(), mask=dm, grad=True, asynchronous=asynchronous)
        torch.cuda.current_stream().synchronize()
        got = {"cost": out["cost"].cpu().numpy(), "grad": out["grad"].cpu().numpy(),
               "maxima": np.ascontiguousarray(out["maxima"].cpu().numpy()).view(EXTREMUM_DTYPE)[..., 0],
               "status": out["status"].cpu().numpy()}
        _same_bits(got, full)


def test_zero_increment_and_bad_times(gpu_ctx):
    N, x, mask, times, prm = M.case("k2")
    p0 = M.Params(prm.constraints, prm.weight, prm.maximum_cost, 0.0)
    out = gpu_ctx.soft_constraint_cost_batch(N, x, times, p0.native(), mask=mask, grad=True)
    n_free = M.model("k2")[0]["n_free"]
    assert np.isfinite(out["cost"]).all() and np.isnan(out["grad"][:, :, :n_free]).all()  # 0 / 0, as the reference
    assert (out["grad"][:, :, n_free:] == 0).all()
    good = _device(gpu_ctx, "k2")
    for badv in (0.0, -1.0, np.inf, np.nan):
        t2 = times.copy()
        t2[1, 1] = badv
        out = gpu_ctx.soft_constraint_cost_batch(N, x, t2, prm.native(), mask=mask, grad=True)
        assert list(out["status"]) == [0, nat.MTG_TRAJ_BAD_TIME, 0, 0, 0]
        assert np.isnan(out["cost"][1]) and (out["grad"][1] == 0).all()
        keep = [0, 2, 3, 4]
        assert out["cost"][keep].tobytes() == good["cost"][keep].tobytes()
        assert out["grad"][keep].tobytes() == good["grad"][keep].tobytes()


def test_too_large_for_lds(gpu_ctx):
    """N = 10, D = 4, two constraints fit up to K = 92 (mtg.h); K = 100 is MTG_ERR_TOO_LARGE, and the host
    path, which has no such limit, still answers."""
    N, K = 10, 100
    values, mask, times = mtg.random_vertices_path_batch(N, 4, K, 1, seed0=3)
    prm = M.Params([(1, 1.0), (2, 1.0)], weight=10.0)
    with pytest.raises(mtg.MTGError) as e:
        gpu_ctx.soft_constraint_cost_batch(N, values, times, prm.native())
    assert e.value.code == nat.MTG_ERR_TOO_LARGE
    out = mtg.host_soft_constraint_cost_batch(N, values, times, prm.native())
    assert out["status"][0] == 0 and out["cost"][0] > 0


@pytest.mark.parametrize("call", list(invalid_calls()), ids=lambda c: c[0])
def test_invalid_arguments(gpu_ctx, call):
    label, N, x, times, prm = call
    with pytest.raises(mtg.MTGError) as e:
        gpu_ctx.soft_constraint_cost_batch(N, x, times, prm.native())
    assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT, label
