"""GPU tests: mtg_cost_at_times_batch (mtg_cost.hip) and mtg_time_jacobian_batch (mtg_jacobian.inc, the
matrix-core kernel) pinned to the 50-digit model of tests/_cost_time_model.py on every code path:
all 21 (N, r) instantiations, the three K buckets of the Jacobian kernel, wide and narrow stores,
ragged and repeated candidate tiles, unstaged scales, streaming stores, the central difference's
floor and NaN rule, the cost-only form, 8-byte-aligned outputs, the cost kernel's candidate and
column loops and its gradient under general masks.

Tolerance (derived, DESIGN.md "Parity"): every compared number is a sum of rounded products, so with
u = 2^-53

    |got - truth| <= (N^2 + 4N + D + K + 16) u S

where S is the sum of the absolute values of the same terms (from the model); for the central
difference [bound(T + dt) + bound(T - dt)] / (2 dt) + 4 u |truth|.  The count is the worst-case
number of roundings a term passes through; nothing in it is measured on the kernels.  Truth is
computed for at most four trajectories per case (first, last, rows 15 and 16 of the first 16-row
tile boundary); the bitwise tests cover the rest.  Each test prints its worst err / bound.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import _cost_time_model as M
from mav_trajectory_generation_cmake_amd import _native as nat

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.1


_RATIOS = []


@pytest.fixture(autouse=True)
def _report_worst_ratio(request):
    """Print the worst err / bound of the test that just ran (the table in DESIGN.md "Parity")."""
    del _RATIOS[:]
    yield
    if _RATIOS:
        print("worst err/bound %s: %.3f" % (request.node.name, max(_RATIOS)))


def _rows(B):
    return sorted({0, B - 1, 15, 16} & set(range(B)))


def _ratio(label, got, truth, bound):
    """Assert |got - truth| <= bound elementwise; returns and prints the worst err / bound."""
    err = M.abs_err(got, truth)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    assert np.all(np.isfinite(got)), label
    assert np.all(err[bound == 0.0] == 0.0), label
    ratio = float(np.max(np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), 0.0))) if err.size else 0.0
    print("err/bound %-34s %.3f" % (label, ratio))
    _RATIOS.append(ratio)
    assert ratio <= 1.0, (label, ratio)
    return ratio


def _check_difference(label, G, ev, cnt):
    """The central difference of one trajectory [C][K] against the model: exactly 0.0 at the floor,
    NaN where the model has NaN, within the bound elsewhere."""
    diff = ev["diff"]
    nan = np.array([[isinstance(v, float) and v != v for v in row] for row in diff])
    zero = np.array([[isinstance(v, float) and v == 0.0 for v in row] for row in diff])
    assert np.array_equal(np.isnan(G), nan), label
    assert np.all(G[zero] == 0.0), label
    live = ~(nan | zero)
    truth = diff[live]
    bound = cnt * M.U * ev["Sdiff"][live] + 4.0 * M.U * np.array([abs(float(v)) for v in truth])
    return _ratio(label, G[live], truth, bound)


def _pin_jacobian(ctx, N, r, vals, times, scales, dts=(0.0, DT), rows=None, label=""):
    """Run the Jacobian kernel (exact and / or central difference) and pin J and the Jacobian of the
    truth rows to the model.  Returns {dt: (J, G)}."""
    B, V, h, D = vals.shape
    K = V - 1
    cnt = M.roundings(N, D, K)
    outs = {dt: ctx.time_jacobian_batch(N, r, vals, times, scales, increment_time=dt) for dt in dts}
    for J, G in outs.values():
        assert J.shape == (B, scales.shape[0]) and G.shape == (B, scales.shape[0], K)
    diff_dts = [dt for dt in dts if dt > 0.0]
    for b in (_rows(B) if rows is None else rows):
        traj = M.Trajectory(N, r, vals[b])
        T = times[b][None, :] * scales
        ev = traj.evaluate(T, dt=diff_dts[0] if diff_dts else None)
        for dt, (J, G) in outs.items():
            tag = "%s b=%d dt=%g" % (label, b, dt)
            _ratio(tag + " J", J[b], ev["J"], cnt * M.U * ev["S"])
            if dt == 0.0:
                _ratio(tag + " dJ/dT", G[b], ev["dJ"], cnt * M.U * ev["Sd"])
            else:
                _check_difference(tag + " diff", G[b], ev, cnt)
    return outs


def _pin_cost(ctx, N, r, vals, mask, times, scales, rows=None, label=""):
    """Run the cost kernel with its gradient and pin J and the packed gradient of the truth rows."""
    B, V, h, D = vals.shape
    K = V - 1
    cnt = M.roundings(N, D, K)
    J, g = ctx.cost_at_times_batch(N, r, vals, times, scales, mask=mask, grad=True)
    n_free = []
    for b in (_rows(B) if rows is None else rows):
        traj = M.Trajectory(N, r, vals[b])
        T = times[b][None, :] * scales
        ev = traj.evaluate(T)
        tag = "%s b=%d cost" % (label, b)
        _ratio(tag + " J", J[b], ev["J"], cnt * M.U * ev["S"])
        gt, Sg, nf = traj.gradient(T, mask[b])
        n_free.append(nf)
        _ratio(tag + " grad", g[b, :, :, :nf], gt, cnt * M.U * Sg)
        assert np.all(g[b, :, :, nf:] == 0.0), tag  # nothing past n_free
    return J, g, n_free


def _random_mask(rng, B, V, h):
    return rng.integers(0, 1 << h, size=(B, V)).astype(np.uint8)


# ---- 1. every instantiation --------------------------------------------------------------------------------
@pytest.mark.parametrize("N,r", M.PAIRS)
def test_all_instantiations(gpu_ctx, N, r):
    """Every (N, r) of both launchers (r = 0 has its own exponent start, N = 2 pads three of four
    k-rows): exact Jacobian, central difference and cost kernel with gradient, against the model."""
    B, K, D, C = 17, 3, 2, 5
    vals, times, scales = M.make_inputs(N, D, K, B, C, seed=100 * N + r)
    mask = _random_mask(np.random.default_rng(N + r), B, K + 1, N // 2)
    outs = _pin_jacobian(gpu_ctx, N, r, vals, times, scales, label="N=%d r=%d" % (N, r))
    Jc, _, _ = _pin_cost(gpu_ctx, N, r, vals, mask, times, scales, label="N=%d r=%d" % (N, r))
    for J, _ in outs.values():
        np.testing.assert_allclose(J, Jc, rtol=1e-11, atol=0)  # the two kernels: same numbers


# ---- 2. K buckets, store widths, tile trips of the Jacobian kernel -----------------------------------------
@pytest.mark.parametrize("N,r,D,K,C", [(10, 4, 3, K, C) for K, C in
                                       [(1, 1), (7, 5), (7, 16), (10, 70), (11, 17), (13, 33), (20, 130), (21, 5),
                                        (25, 17), (25, 70)]] + [(12, 3, 2, 25, 17), (2, 0, 1, 7, 5)])
def test_jacobian_k_and_c_paths(gpu_ctx, N, r, D, K, C):
    """KMAX 10 / 20 / 0 (K <= 10, <= 20, above), 16-byte and 8-byte stores (narrow exactly when K and C
    are odd), ragged last candidate tiles, second and third tile trips of a wave (C > 64, > 128)."""
    vals, times, scales = M.make_inputs(N, D, K, 17, C, seed=1000 * K + C)
    _pin_jacobian(gpu_ctx, N, r, vals, times, scales, label="K=%d C=%d" % (K, C))


# ---- 3. other dimensions and small batches -----------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 4, 6])
def test_jacobian_dimensions(gpu_ctx, D):
    vals, times, scales = M.make_inputs(8, D, 6, 17, 9, seed=40 + D)
    _pin_jacobian(gpu_ctx, 8, 2, vals, times, scales, label="D=%d" % D)


@pytest.mark.parametrize("B", [1, 15, 16, 33])
def test_jacobian_small_batches(gpu_ctx, B):
    """Fewer rows than one 16-row tile, exactly one tile, a ragged third tile (config-2 shape)."""
    vals, times, scales = M.make_inputs(10, 3, 10, B, 20, seed=50 + B)
    _pin_jacobian(gpu_ctx, 10, 4, vals, times, scales, label="B=%d" % B)


# ---- 4. rows and columns do not mix ------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0.0, DT])
@pytest.mark.parametrize("K", [7, 10, 25])
def test_rows_and_columns_independent_bitwise(gpu_ctx, K, dt):
    """One trajectory repeated 33 times gives 33 bit-identical rows; one candidate repeated 70 times
    gives 70 bit-identical columns (any cross-lane or cross-tile mix-up of the MFMA operands or of
    the waves' store buffers breaks one of the two)."""
    N, r, D = 10, 4, 3
    vals, times, scales = M.make_inputs(N, D, K, 33, 37, seed=7 + K)
    J, G = gpu_ctx.time_jacobian_batch(N, r, np.repeat(vals[:1], 33, axis=0), np.repeat(times[:1], 33, axis=0), scales,
                                       increment_time=dt)
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(G))
    np.testing.assert_array_equal(J, np.repeat(J[:1], 33, axis=0))
    np.testing.assert_array_equal(G, np.repeat(G[:1], 33, axis=0))
    J, G = gpu_ctx.time_jacobian_batch(N, r, vals[:17], times[:17], np.repeat(scales[1:2], 70, axis=0),
                                       increment_time=dt)
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(G))
    np.testing.assert_array_equal(J, np.repeat(J[:, :1], 70, axis=1))
    np.testing.assert_array_equal(G, np.repeat(G[:, :1], 70, axis=1))


def _source_constant(name):
    """A size constant of mtg_jacobian.inc, so that a test built around it notices when it moves."""
    with open(os.path.join(ROOT, "mav_trajectory_generation_cmake_amd", "csrc", "mtg_jacobian.inc")) as f:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, f.read())
    expr = re.sub(r"\(\s*size_t\s*\)", "", m.group(1))
    assert re.fullmatch(r"[\d\s<>*+()]+", expr), expr
    return int(eval(expr))


# ---- 5. candidate scales read from global memory -----------------------------------------------------------
@pytest.mark.parametrize("K,C", [(20, 205), (25, 164)])
def test_unstaged_scales(gpu_ctx, K, C):
    """C K above kJacScalesMax: the scales are read from global memory, not from LDS.  Bit-identical to
    the same candidates sent as two calls that stage them; two trajectories pinned to the model."""
    N, r, D, B = 10, 4, 3, 17
    limit = _source_constant("kJacScalesMax")
    assert limit == 4096
    C1 = C // 2
    assert C * K > limit and C1 * K <= limit and (C - C1) * K <= limit
    vals, times, scales = M.make_inputs(N, D, K, B, C, seed=3 * K)
    outs = _pin_jacobian(gpu_ctx, N, r, vals, times, scales, rows=[0, 16], label="unstaged K=%d" % K)
    for dt, (J, G) in outs.items():
        Ja, Ga = gpu_ctx.time_jacobian_batch(N, r, vals, times, scales[:C1], increment_time=dt)
        Jb, Gb = gpu_ctx.time_jacobian_batch(N, r, vals, times, scales[C1:], increment_time=dt)
        np.testing.assert_array_equal(J, np.concatenate([Ja, Jb], axis=1))
        np.testing.assert_array_equal(G, np.concatenate([Ga, Gb], axis=1))


# ---- 6. streaming stores -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,C", [(4200, 16, 128), (4400, 15, 129)])
def test_streaming_stores(gpu_ctx, B, K, C):
    """A Jacobian above kJacSc1MaxBytes leaves with streaming stores (16-byte for even C K, 8-byte for
    K and C odd), below it with sc1 buffer stores: bit-identical to the same batch sent as two halves,
    four trajectories pinned to the model."""
    N, r, D = 6, 2, 1
    limit = _source_constant("kJacSc1MaxBytes")
    assert limit == 64 << 20
    assert B * C * K * 8 > limit and (B // 2) * C * K * 8 <= limit and B % 2 == 0
    assert ((K * C) % 2 == 1) == (K == 15)
    vals, times, scales = M.make_inputs(N, D, K, B, C, seed=B)
    outs = _pin_jacobian(gpu_ctx, N, r, vals, times, scales, dts=(0.0,), label="streaming K=%d" % K)
    J, G = outs[0.0]
    h = B // 2
    for lo, hi in ((0, h), (h, B)):
        Jh, Gh = gpu_ctx.time_jacobian_batch(N, r, vals[lo:hi], times[lo:hi], scales)
        np.testing.assert_array_equal(J[lo:hi], Jh)
        np.testing.assert_array_equal(G[lo:hi], Gh)
    Jd, Gd = gpu_ctx.time_jacobian_batch(N, r, vals, times, scales, increment_time=DT)
    Jh, Gh = gpu_ctx.time_jacobian_batch(N, r, vals[h:], times[h:], scales, increment_time=DT)
    np.testing.assert_array_equal(Jd[h:], Jh)
    np.testing.assert_array_equal(Gd[h:], Gh)


# ---- 7. the cost-only form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0.0, DT])
@pytest.mark.parametrize("K", [10, 25])
def test_cost_only_form(gpu_ctx, K, dt):
    """jac_out == NULL: the same J, bit for bit, as the call that also writes the Jacobian."""
    vals, times, scales = M.make_inputs(10, 3, K, 17, 21, seed=70 + K)
    J, _ = gpu_ctx.time_jacobian_batch(10, 4, vals, times, scales, increment_time=dt)
    Jo = gpu_ctx.time_jacobian_batch(10, 4, vals, times, scales, increment_time=dt, jacobian=False)
    assert np.all(np.isfinite(J))
    np.testing.assert_array_equal(J, Jo)


# ---- 8. the central difference's floor and NaN rule --------------------------------------------------------
def test_time_edges(gpu_ctx):
    """dt = 0.5: a candidate time of 0.3 (above the 0.1 floor, T - dt <= 0) gives NaN in exactly that
    entry, 0.08 and exactly 0.1 give exactly 0.0; every other entry and every J is finite and within
    the bound."""
    N, r, D, K, B, C = 10, 4, 3, 10, 17, 5
    dt = 0.5
    vals, times, scales = M.make_inputs(N, D, K, B, C, seed=8)
    times = np.maximum(times, 1.2)  # x 0.5 (the smallest scale) stays above dt
    times[0, 3], times[16, 0], times[15, 9] = 0.3, 0.08, 0.1
    Tc = times[:, None, :] * scales[None, :, :]
    want_nan = (Tc > 0.1) & (Tc - dt <= 0.0)
    want_zero = Tc <= 0.1
    assert want_nan[0, 0, 3] and want_zero[16, 0, 0] and want_zero[15, 0, 9]
    assert want_nan[:, 0].sum() == 1 and want_zero[:, 0].sum() == 2  # candidate 0 has scales of 1
    outs = _pin_jacobian(gpu_ctx, N, r, vals, times, scales, dts=(dt,), label="edges")
    J, G = outs[dt]
    assert np.all(np.isfinite(J))
    np.testing.assert_array_equal(np.isnan(G), want_nan)
    np.testing.assert_array_equal(G == 0.0, want_zero)
    assert np.all(np.isfinite(G[~want_nan]))


# ---- 9. device outputs at 8-byte alignment -----------------------------------------------------------------
@pytest.mark.parametrize("K,C", [(10, 20), (7, 5)])
def test_outputs_only_8_byte_aligned(gpu_ctx, K, C):
    """cost and jac at addresses that are 8 mod 16 (the 16-byte store path has no alignment term):
    bit-identical to the aligned call, guard words before and after untouched."""
    import torch
    N, r, D, B = 10, 4, 3, 17
    vals, times, scales = M.make_inputs(N, D, K, B, C, seed=90 + K)
    dev = torch.device("cuda", 0)
    v_d, t_d, s_d = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (vals, times, scales))

    def buffers(shift):
        bufs = [torch.full((n + 2 + shift,), np.nan, dtype=torch.float64, device=dev) for n in (B * C, B * C * K)]
        return bufs, [b[1 + shift:-1] for b in bufs]

    for dt in (0.0, DT):
        (_, _), (c_ref, j_ref) = buffers(1)
        assert c_ref.data_ptr() % 16 == 0 and j_ref.data_ptr() % 16 == 0
        gpu_ctx.jacobian_call(N, r, v_d, t_d, s_d, c_ref, j_ref, increment_time=dt)()
        (bc, bj), (c_out, j_out) = buffers(0)
        assert c_out.data_ptr() % 16 == 8 and j_out.data_ptr() % 16 == 8
        gpu_ctx.jacobian_call(N, r, v_d, t_d, s_d, c_out, j_out, increment_time=dt)()
        torch.cuda.synchronize()
        assert np.all(np.isfinite(j_ref.cpu().numpy())) and np.all(np.isfinite(c_ref.cpu().numpy()))
        np.testing.assert_array_equal(c_out.cpu().numpy(), c_ref.cpu().numpy())
        np.testing.assert_array_equal(j_out.cpu().numpy(), j_ref.cpu().numpy())
        for b in (bc, bj):
            assert np.isnan(b[0].item()) and np.isnan(b[-1].item())
    (_, _), (c_ref, _) = buffers(1)
    gpu_ctx.cost_call(N, r, v_d, t_d, s_d, c_ref)()
    (bc, _), (c_out, _) = buffers(0)
    gpu_ctx.cost_call(N, r, v_d, t_d, s_d, c_out)()
    torch.cuda.synchronize()
    assert np.all(np.isfinite(c_ref.cpu().numpy()))
    np.testing.assert_array_equal(c_out.cpu().numpy(), c_ref.cpu().numpy())
    assert np.isnan(bc[0].item()) and np.isnan(bc[-1].item())
    gpu_ctx.reset_stream()


# ---- 10. the cost kernel's loops ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,r,K,C", [(10, 4, 10, 65), (10, 4, 10, 130), (10, 4, 25, 5), (12, 3, 100, 3)])
def test_cost_kernel_loops(gpu_ctx, N, r, K, C):
    """Second and third trip of the candidate loop (C > 64, > 128) and of the column loop
    (K D = 75, 300 > 64), J and gradient against the model (trajectory 1 carries the position offset)."""
    B, D = 3, 3
    vals, times, scales = M.make_inputs(N, D, K, B, C, seed=K + C)
    mask = _random_mask(np.random.default_rng(K * C), B, K + 1, N // 2)
    _pin_cost(gpu_ctx, N, r, vals, mask, times, scales, rows=[0, 1, 2], label="K=%d C=%d" % (K, C))


# ---- 11. the gradient under general masks ------------------------------------------------------------------
def test_cost_gradient_general_masks(gpu_ctx):
    """Masks drawn per trajectory, with a fully free interior vertex, a fully fixed interior vertex, a
    free order at the start vertex and n_free differing inside the batch: the packed gradient in the
    reference's free order, exactly 0.0 from n_free on."""
    N, r, K, D, B, C = 10, 4, 6, 3, 9, 5
    h = N // 2
    vals, times, scales = M.make_inputs(N, D, K, B, C, seed=11)
    mask = _random_mask(np.random.default_rng(12), B, K + 1, h)
    mask[0, 2] = 0
    mask[1, 3] = (1 << h) - 1
    mask[2, 0] = 0b11101
    mask[B - 1] = 0b00001
    _, _, n_free = _pin_cost(gpu_ctx, N, r, vals, mask, times, scales, rows=[0, 1, 2, B - 1], label="masks")
    assert len(set(n_free)) > 1, n_free
    assert n_free[-1] == (K + 1) * (h - 1)


# ---- 12. host-side rejections (no kernel is launched) ------------------------------------------------------
def test_host_side_rejections(gpu_ctx):
    lib = gpu_ctx._lib
    gpu_ctx.reset_stream()

    def call(N, D, K, r, B, C, dt, Balloc=1):
        h = N // 2
        vals = np.zeros((Balloc, K + 1, h, D))
        times = np.ones((Balloc, K))
        scales = np.ones((max(C, 1), K))
        cost = np.full((Balloc, max(C, 1)), np.nan)
        jac = np.full((Balloc, max(C, 1), K), np.nan)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = lib.mtg_time_jacobian_batch(gpu_ctx.handle, N, D, K, r, B, p(vals), p(times), C, p(scales), dt, p(cost),
                                         p(jac), 0)
        assert np.all(np.isnan(cost)) and np.all(np.isnan(jac))  # nothing was written
        return rc

    assert call(12, 3, 40, 3, 1, 4, 0.0) == nat.MTG_ERR_TOO_LARGE
    assert call(10, 3, 10, 4, 1, 0, 0.0) == nat.MTG_ERR_SIZE_MISMATCH
    assert call(10, 3, 10, 4, 1, 4, -0.1) == nat.MTG_ERR_INVALID_ARGUMENT
    assert call(10, 3, 10, 4, 1, 4, float("nan")) == nat.MTG_ERR_INVALID_ARGUMENT
    assert call(10, 3, 10, 4, 0, 4, 0.0) == nat.MTG_OK
    with open(os.path.join(ROOT, "include", "mtg.h")) as f:
        header = f.read()
    for name in ("MTG_OK", "MTG_ERR_INVALID_ARGUMENT", "MTG_ERR_SIZE_MISMATCH", "MTG_ERR_TOO_LARGE"):
        m = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, header)
        assert m and int(m.group(1)) == getattr(nat, name), name
