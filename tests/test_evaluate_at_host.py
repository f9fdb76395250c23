"""mtg_host_evaluate_at_batch (the host path of mtg_evaluate_at_batch, include/mtg.h) against the
definition in numpy (tests/_evaluate_at_model.py), bit for bit, and against the oracle's evaluateRange.
CPU only."""
import itertools

import numpy as np
import pytest

import _evaluate_at_model as model
from mav_trajectory_generation_cmake_amd import _native as nat
from mav_trajectory_generation_cmake_amd import host_evaluate_at_batch

NS, DS, KS, BS, MS = (2, 6, 10, 12), (1, 3, 4, 5), (1, 2, 10, 37), (1, 7), (1, 3, 65)
STRIDES = ("shared", "dense", "padded")  # t_stride 0, M, M + 3


def strided_queries(tq, kind):
    """The query times as the entry sees them: one shared row (trajectory 0's), [B][M], or a view of a
    [B][M + 3] buffer whose padding is NaN."""
    if kind == "shared":
        return tq[0].copy()
    if kind == "dense":
        return tq
    buf = np.full((tq.shape[0], tq.shape[1] + 3), np.nan)
    buf[:, :tq.shape[1]] = tq
    return buf[:, :tq.shape[1]]


def check_against_model(coeffs, times, tq, k0, nd, what):
    got = host_evaluate_at_batch(coeffs, times, tq, k0, nd)
    want = model.evaluate_at(coeffs, times, tq, k0, nd)
    model.assert_same_bits(got[0], want[0], what)
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[2], want[2]), what
    return got


@pytest.mark.parametrize("N", NS)
def test_bitwise_vs_model(N):
    """Every (D, K, B, M) at this N with every derivative pair and every stride."""
    rng = np.random.default_rng(1000 + N)
    for D, K, B, M in itertools.product(DS, KS, BS, MS):
        coeffs, times, tq = model.random_case(rng, N, D, K, B, M)
        for (k0, nd), kind in itertools.product(model.derivative_pairs(N), STRIDES):
            check_against_model(coeffs, times, strided_queries(tq, kind), k0, nd, (N, D, K, B, M, k0, nd, kind))


@pytest.mark.parametrize("N", NS)
def test_every_pair_and_stride_at_one_shape(N):
    rng = np.random.default_rng(2000 + N)
    coeffs, times, tq = model.random_case(rng, N, 3, 10, 7, 65)
    for (k0, nd), kind in itertools.product(model.derivative_pairs(N), STRIDES):
        got = check_against_model(coeffs, times, strided_queries(tq, kind), k0, nd, (N, k0, nd, kind))
        if k0 >= N:
            assert not got[0].any() and not np.signbit(got[0]).any()  # +0.0


@pytest.mark.parametrize("N,D,K", [(10, 3, 10), (2, 5, 2), (6, 1, 1), (12, 4, 37)])
def test_edge_case_times(N, D, K):
    """t = 0, t < 0, every interior prefix value (the segment to the right), the total and its neighbours,
    +inf (zeros, out of range), -inf and NaN, for every trajectory."""
    rng = np.random.default_rng(3000 + N + K)
    B = 7
    coeffs, times, _ = model.random_case(rng, N, D, K, B, 1)
    tq = np.stack([model.edge_times(times[b]) for b in range(B)])
    for k0, nd in model.derivative_pairs(N):
        out, in_range, status = check_against_model(coeffs, times, tq, k0, nd, (N, D, K, k0, nd))
        assert not status.any()
    out, in_range, _ = host_evaluate_at_batch(coeffs, times, tq, 0, 1)
    M = tq.shape[1]
    i_total = 2 + (K - 1)
    want_in = np.ones(M, np.uint8)
    want_in[[i_total + 1, M - 3, M - 1]] = 0  # just beyond the total, +inf, NaN
    assert (in_range == want_in[None, :]).all()
    assert not out[:, [i_total + 1, M - 3]].any()
    assert np.isnan(out[:, M - 1]).all()


def test_independent_check_against_the_oracle():
    """oracle.pyoracle.evaluate_range started at t runs the same search and the same t - (acc - T_i); its
    first sample is the entry's row.  t_end is the double just above t and dt = 1, every chosen t must
    give a sample."""
    from oracle import pyoracle
    rng = np.random.default_rng(4)
    for N, D, K in ((10, 3, 10), (6, 1, 2), (12, 4, 37)):
        B, M = 3, 17
        coeffs, times, tq = model.random_case(rng, N, D, K, B, M)
        for k in (0, 1, 2, N - 1):
            out, in_range, _ = host_evaluate_at_batch(coeffs, times, tq, k, 1)
            assert in_range.all()
            for b in range(B):
                for m in range(M):
                    t = float(tq[b, m])
                    samples, _, n = pyoracle.evaluate_range(coeffs[b], times[b], t, float(np.nextafter(t, np.inf)), 1.0,
                                                            derivative=k, max_samples=4)
                    assert n >= 1, (N, K, b, m, t)
                    model.assert_same_bits(out[b, m, 0], samples[0], (N, K, b, m, k))


def test_the_inputs_can_see_an_fma():
    """A model with every Horner step fused differs from the definition in at least one bit of at least
    1 % of the rows of these tests' inputs, so a contracted build cannot pass by luck."""
    rng = np.random.default_rng(2000 + 10)  # the inputs of test_every_pair_and_stride_at_one_shape, N = 10
    coeffs, times, tq = model.random_case(rng, 10, 3, 10, 7, 65)
    plain = model.evaluate_at(coeffs, times, tq, 0, 3)[0]
    fused = model.evaluate_at(coeffs, times, tq, 0, 3, fused=True)[0]
    rows = (plain.view(np.uint64) != fused.view(np.uint64)).reshape(7 * 65, -1).any(axis=1)
    assert rows.mean() >= 0.01, rows.mean()
    model.assert_same_bits(host_evaluate_at_batch(coeffs, times, tq, 0, 3)[0], plain)


def test_bad_times():
    rng = np.random.default_rng(5)
    N, D, K, B, M = 10, 3, 10, 8, 9
    coeffs, times, tq = model.random_case(rng, N, D, K, B, M)
    bad = {1: 0.0, 4: -1.0, 6: np.nan}
    for b, v in bad.items():
        times[b, 3] = v
    out, in_range, status = check_against_model(coeffs, times, tq, 0, 3, "bad times")
    good = [b for b in range(B) if b not in bad]
    for b in bad:
        assert status[b] == nat.MTG_TRAJ_BAD_TIME and np.isnan(out[b]).all() and not in_range[b].any()
    assert not status[good].any() and in_range[good].all()
    alone = host_evaluate_at_batch(coeffs[good], times[good], tq[good], 0, 3)
    model.assert_same_bits(out[good], alone[0])
    times[2, 0] = np.inf
    assert host_evaluate_at_batch(coeffs, times, tq, 0, 1)[2][2] == nat.MTG_TRAJ_BAD_TIME


def test_argument_errors():
    lib = nat.load()
    N, D, K, B, M = 10, 3, 4, 2, 5
    c, t, q = np.zeros((B, K, D, N)), np.ones((B, K)), np.zeros((B, M))
    out = np.full((B, M, 3, D), 7.0)

    def call(N=N, D=D, K=K, B=B, c=c, t=t, q=q, stride=M, M=M, k0=0, nd=3, out=out):
        a = [x.ctypes.data if x is not None else None for x in (c, t, q, out)]
        return lib.mtg_host_evaluate_at_batch(N, D, K, B, a[0], a[1], a[2], stride, M, k0, nd, a[3], None, None, 1)

    assert call() == nat.MTG_OK
    for bad_n in (0, 3, 11, 14):
        assert call(N=bad_n) == nat.MTG_ERR_UNSUPPORTED_N
    assert call(K=0) == call(D=0) == call(B=-1) == call(M=-1, stride=0) == nat.MTG_ERR_SIZE_MISMATCH
    assert call(k0=-1) == call(nd=0) == call(nd=N + 1) == nat.MTG_ERR_BAD_DERIVATIVE
    assert call(nd=N, out=np.zeros((B, M, N, D))) == nat.MTG_OK
    assert call(stride=M - 1) == call(stride=1) == call(stride=-1) == nat.MTG_ERR_INVALID_ARGUMENT
    assert call(c=None) == call(t=None) == call(q=None) == call(out=None) == nat.MTG_ERR_INVALID_ARGUMENT
    out[:] = 7.0
    assert call(B=0) == call(M=0, stride=0) == call(B=0, c=None, t=None, q=None, out=None) == nat.MTG_OK
    assert (out == 7.0).all()  # nothing written
    # the device entry reports the same argument errors before it needs a device (a null context first)
    a = [x.ctypes.data for x in (c, t, q, out)]
    assert lib.mtg_evaluate_at_batch(None, N, D, K, B, a[0], a[1], a[2], M, M, 0, 3, a[3], None, None,
                                     0) == nat.MTG_ERR_INVALID_ARGUMENT
    assert lib.mtg_evaluate_at_path(11, 3, 10, 1, 1) == nat.MTG_ERR_UNSUPPORTED_N
    assert lib.mtg_evaluate_at_path(10, 3, 10, 1, 11) == nat.MTG_ERR_BAD_DERIVATIVE
    assert lib.mtg_evaluate_at_path(10, 0, 10, 1, 1) == nat.MTG_ERR_SIZE_MISMATCH
    assert lib.mtg_evaluate_at_path(12, 11, 10, 1, 12) == nat.MTG_ERR_TOO_LARGE  # 132 doubles per row


def test_path_rule_depends_on_the_shape_only():
    """Staged iff M >= max(32, K) and the staged block fits LDS."""
    lane, staged = nat.MTG_EVALUATE_AT_LANE, nat.MTG_EVALUATE_AT_STAGED
    assert nat.evaluate_at_path(10, 3, 10, 1) == lane
    assert nat.evaluate_at_path(10, 3, 10, 31, 3) == lane
    assert nat.evaluate_at_path(10, 3, 10, 32, 3) == staged
    assert nat.evaluate_at_path(10, 3, 100, 99) == lane
    assert nat.evaluate_at_path(10, 3, 100, 100) == staged
    assert nat.evaluate_at_path(12, 4, 100, 300, 3) == staged
    assert nat.evaluate_at_path(12, 4, 100, 300, 12) == staged  # 64 threads: 64584 bytes of LDS
    assert nat.evaluate_at_path(12, 4, 120, 300, 12) == lane    # the staged block would pass 64 KiB
    assert nat.evaluate_at_path(12, 4, 100, 1, 12) == lane      # K <= 100 at N = 12, D = 4 always fits


def test_kernels_have_no_fma(tmp_path):
    """The gfx950 code of both kernels, every N: no f64 FMA, so no contracted Horner step (HIP contracts
    by default; the kernels say `fp contract(off)`)."""
    import os
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "mav_trajectory_generation_cmake_amd", "csrc")
    out = tmp_path / "mtg_evaluate_at.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I",
                    os.path.join(root, "include"), "-I", csrc, os.path.join(csrc, "mtg_evaluate_at.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    asm = out.read_text()
    kernels = re.findall(r"^(_ZN3mtg\w*evaluate_at_\w+_kernel\w*):", asm, flags=re.M)
    assert len(kernels) == 12, kernels  # (lane, staged) x N = 2, 4, ..., 12
    assert "v_mul_f64" in asm and "v_add_f64" in asm
    assert not re.search(r"v_fmac?_f64", asm)
    assert re.findall(r"\.private_segment_fixed_size: (\d+)", asm) == ["0"] * 12  # no scratch


def test_thread_independence():
    rng = np.random.default_rng(6)
    coeffs, times, tq = model.random_case(rng, 10, 3, 10, 50, 9)
    one = host_evaluate_at_batch(coeffs, times, tq, 0, 3, threads=1)
    dflt = host_evaluate_at_batch(coeffs, times, tq, 0, 3, threads=0)
    model.assert_same_bits(one[0], dflt[0])
    assert np.array_equal(one[1], dflt[1]) and np.array_equal(one[2], dflt[2])
