"""mtg_evaluate_range_ragged_batch / mtg_evaluate_range_ragged_batch_full (csrc/mtg_eval_ragged.hip: the
kernels of mtg_eval.inc with the CSR indirection) against the sequential restatement of
Trajectory::evaluateRange (oracle.pyoracle.evaluate_range) called per trajectory with that trajectory's
K_b.  Every comparison is bit equality: counts, offsets, total, every sample row and every sample time,
through the two-call and the one-call form, with and without sample times.

  case 1   mixed K inside and across a clock wave; slices and a permutation of the batch
  case 2   equal K: the uniform entries' bytes
  case 3   window edges with empty neighbours; the uniform suite's clock edges at mixed K
  case 4   a run table that overflows next to stored clocks (D = 2: lane 0 resumes; D = 3: `rest`)
  case 5   the sample kernels' LDS thresholds by K_max, and the clean error past them
  case 6   both clock variants by the staging rule (segment times in LDS / from global memory)
  case 7   the ragged solve's device outputs passed straight in
  case 8   the one-call protocol (capacity exact, short, DEVICE_PTRS | ASYNC)
  case 9   two asynchronous calls with different seg_count back to back
  case 10  argument errors and batch = 0

Each case asserts on the CPU, before the GPU call, that its inputs reach the path it is there for (the
run model and LDS formulas of test_gpu_evaluate_range.py, the staging rule restated here), that its batch
has a K_b that differs from its neighbour's, and that every trajectory has at least one sample unless
the case names it as empty: a trajectory is empty exactly when t_start lies beyond its accumulated
duration (Trajectory::evaluateRange then returns nothing), which `empties` computes from the inputs."""
import time

import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat
from test_gpu_evaluate_range import (CLOCK_EDGES, CLOCK_LDS_K, LDS_MAX, RUN_TABLE, SENTINEL, T_END_OPEN, _Ref, _compare,
                                     _lds, _lds_pc, _oracle, _runs, _same_bits, _segments_crossed)

pytestmark = pytest.mark.gpu

PAIR_TRAJ = 32  # kPairTraj: trajectories per wave of the clock kernels


# ------------------------------------------------------------------ inputs
def _blocks(seed, Ks, D, N, lo, hi):
    """Per trajectory: seeded normal coefficients [K_b][D][N] and uniform times [K_b] in [lo, hi]; every
    third trajectory has an all-zero segment and a -0.0 entry."""
    rng = np.random.default_rng(seed)
    cl, tl = [], []
    for b, K in enumerate(Ks):
        c = rng.standard_normal((K, D, N))
        if b % 3 == 0:
            c[b % K] = 0.0
            c[(b + 1) % K, b % D, b % N] = -0.0
        cl.append(c)
        tl.append(rng.uniform(lo, hi, K))
    return cl, tl


def _csr(cl, tl):
    return (np.ascontiguousarray(np.concatenate(cl)), np.ascontiguousarray(np.concatenate(tl)),
            np.array([len(t) for t in tl], dtype=np.int32))


def _reference(cl, tl, ts, te, dt, der):
    """The oracle on every trajectory, each with its own K_b."""
    O = _oracle()
    rows = []
    for c, t in zip(cl, tl):
        c, t = np.ascontiguousarray(c), np.ascontiguousarray(t)
        n = O.evaluate_range(c, t, ts, te, dt, der, max_samples=0)[2]
        assert 0 <= n <= 200000, "a case of this module never has this many samples: %d" % n
        out, st, n2 = O.evaluate_range(c, t, ts, te, dt, der, max_samples=max(n, 1))
        assert n2 == n
        rows.append((out[:n].copy(), st[:n].copy()))
    return _Ref(rows, cl[0].shape[1])


def empties(tl, ts):
    """The trajectories the case names as empty: t_start beyond the accumulated duration (left-to-right sum)."""
    return {b for b, t in enumerate(tl) if ts > float(np.cumsum(t)[-1])}


def _conditions(tl, ts, ref, equal_k=False):
    Ks = [len(t) for t in tl]
    if len(Ks) > 1 and not equal_k:
        assert any(a != b for a, b in zip(Ks, Ks[1:])), "no K_b differs from its neighbour"
    named = empties(tl, ts)
    for b in range(len(tl)):
        assert (ref.counts[b] == 0) == (b in named), (b, ref.counts[b], sorted(named))


def clock_slice(Ks):
    """eval_ragged_clock_slice: the most segments of any 32-trajectory block of the clock kernels."""
    return max(sum(Ks[b0:b0 + PAIR_TRAJ]) for b0 in range(0, len(Ks), PAIR_TRAJ))


def clock_staged(Ks):
    """The staging rule of include/mtg.h: segment times in LDS iff the largest slice fits 32 * 256 doubles."""
    return clock_slice(Ks) <= PAIR_TRAJ * CLOCK_LDS_K


# ------------------------------------------------------------------ every form of the call
def _check(ctx, name, cl, tl, ts, te, dt, der=0, ref=None, device=False, misaligned=False, equal_k=False):
    """Two-call and one-call form from numpy arrays, each with and without sample times; device: the
    one-call form from device tensors; misaligned: the two-call form's sample call, device pointers, into
    an output that is only 8-B aligned."""
    if ref is None:
        ref = _reference(cl, tl, ts, te, dt, der)
    _conditions(tl, ts, ref, equal_k)
    coeffs, times, seg = _csr(cl, tl)
    B, D, N = len(seg), coeffs.shape[1], coeffs.shape[2]
    t0 = time.perf_counter()
    for wt in (True, False):
        got = ctx.evaluate_range_ragged_batch(coeffs, times, seg, ts, te, dt, der, want_times=wt)
        _compare("%s two-call%s" % (name, "" if wt else " no times"), got, ref, wt)
        got = ctx.evaluate_range_ragged_batch_full(coeffs, times, seg, ts, te, dt, der, want_times=wt,
                                                   capacity=ref.total)
        _compare("%s one-call%s" % (name, "" if wt else " no times"), got, ref, wt)
    if device or misaligned:
        import torch
        from mav_trajectory_generation_cmake_amd.solver import _addr
        c_d, t_d = torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda()
    if device:
        for wt in (True, False):
            got = ctx.evaluate_range_ragged_batch_full(c_d, t_d, seg, ts, te, dt, der, want_times=wt, capacity=ref.total)
            torch.cuda.synchronize()
            got = tuple(None if g is None else g.cpu().numpy() for g in got)
            _compare("%s one-call device%s" % (name, "" if wt else " no times"), got, ref, wt)
    if misaligned and ref.total > 0:
        cnt_d, off_d = torch.from_numpy(ref.counts).cuda(), torch.from_numpy(ref.offsets).cuda()
        for wt in (True, False):
            buf = torch.full((ref.total * D + 2,), SENTINEL, dtype=torch.float64, device="cuda")
            view = buf[1:-1]
            assert view.data_ptr() % 16 == 8
            st_d = torch.full((ref.total + 1,), SENTINEL, dtype=torch.float64, device="cuda") if wt else None
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            nat.check(ctx._lib.mtg_evaluate_range_ragged_batch(ctx.handle, N, D, B, _addr(seg), _addr(c_d), _addr(t_d),
                                                               float(ts), float(te), float(dt), int(der), _addr(cnt_d),
                                                               _addr(off_d), _addr(view), _addr(st_d) if wt else None,
                                                               nat.MTG_FLAG_DEVICE_PTRS), ctx.handle)
            torch.cuda.synchronize()
            assert buf[0].item() == SENTINEL and buf[-1].item() == SENTINEL
            _same_bits(name + " 8-B aligned samples", view.cpu().numpy().reshape(ref.total, D), ref.out, ref)
            if wt:
                assert st_d[-1].item() == SENTINEL
                _same_bits(name + " 8-B aligned sample times", st_d[:-1].cpu().numpy(), ref.st, ref)
    ctx.reset_stream()
    print("ragged evaluateRange %s: N=%d D=%d B=%d K=%d..%d derivative=%d total=%d samples, device calls %.3f s"
          % (name, N, D, B, seg.min(), seg.max(), der, ref.total, time.perf_counter() - t0))
    return ref


# ------------------------------------------------------------------ case 1
def _mixed_ks(B=65, seed=11):
    Ks = np.random.default_rng(seed).choice([1, 2, 3, 5, 8, 13], size=B)
    Ks[[0, 31, 32, 64]] = 1
    return [int(k) for k in Ks]


@pytest.fixture(scope="module", params=[3, 2])
def mixed(request):
    D = request.param
    Ks = _mixed_ks()
    cl, tl = _blocks(100 + D, Ks, D, 10, 0.3, 1.5)
    ref = _reference(cl, tl, 0.0, T_END_OPEN, 0.01, 0)
    return dict(D=D, Ks=Ks, cl=cl, tl=tl, ref=ref)


def test_mixed_k_inputs(mixed):
    """K = 1 at the first and last lane pair of a wave and alone in the third wave; every value of
    {1, 2, 3, 5, 8, 13} occurs in both full waves; one staged slice per wave."""
    Ks = mixed["Ks"]
    assert [Ks[b] for b in (0, 31, 32, 64)] == [1, 1, 1, 1]
    assert set(Ks[:32]) == set(Ks[32:64]) == {1, 2, 3, 5, 8, 13}
    assert clock_staged(Ks) and mixed["ref"].counts.min() >= 30


@pytest.mark.parametrize("lo,hi", [(0, 65), (0, 1), (1, 2), (0, 31), (0, 32), (0, 33)])
def test_mixed_k_and_slices(gpu_ctx, mixed, lo, hi):
    """N = 10, B = 65, times in [0.3, 1.5], dt = 0.01, [0, open end), and the slices of the same batch: a
    trajectory's bytes are the oracle's for it alone, so they equal its bytes in the full batch.  (The
    slices of one trajectory cannot have a differing neighbour.)  D = 3: eval_range_pc_kernel; D = 2:
    eval_range_kernel<10, 0, 0, false>."""
    m = mixed
    _check(gpu_ctx, "mixed[%d:%d]" % (lo, hi), m["cl"][lo:hi], m["tl"][lo:hi], 0.0, T_END_OPEN, 0.01, 0,
           ref=m["ref"].head(lo, hi, m["D"]), device=(lo, hi) == (0, 65), misaligned=(lo, hi) == (0, 33))


def test_mixed_k_permuted(gpu_ctx, mixed):
    """A permutation of the batch gives the permuted blocks."""
    m = mixed
    perm = np.random.default_rng(12).permutation(65)
    cl, tl = [m["cl"][j] for j in perm], [m["tl"][j] for j in perm]
    _check(gpu_ctx, "mixed permuted", cl, tl, 0.0, T_END_OPEN, 0.01, 0, ref=_Ref([m["ref"].rows[j] for j in perm], m["D"]))


# ------------------------------------------------------------------ case 2
@pytest.mark.parametrize("D", [3, 2])
def test_equal_k_equals_the_uniform_entries(gpu_ctx, D):
    """All K_b = 6, B = 34: every output of the ragged entries equals the uniform entries' byte for byte
    (and the oracle's)."""
    B, K, N = 34, 6, 10
    cl, tl = _blocks(200 + D, [K] * B, D, N, 0.3, 1.5)
    ref = _check(gpu_ctx, "equal K", cl, tl, 0.2, 5.0, 0.01, 1, equal_k=True, device=True)
    coeffs, times, seg = _csr(cl, tl)
    cu, tu = coeffs.reshape(B, K, D, N), times.reshape(B, K)
    for wt in (True, False):
        want = gpu_ctx.evaluate_range_batch(cu, tu, 0.2, 5.0, 0.01, 1, want_times=wt)
        got = gpu_ctx.evaluate_range_ragged_batch(coeffs, times, seg, 0.2, 5.0, 0.01, 1, want_times=wt)
        want_f = gpu_ctx.evaluate_range_batch_full(cu, tu, 0.2, 5.0, 0.01, 1, want_times=wt, capacity=ref.total)
        got_f = gpu_ctx.evaluate_range_ragged_batch_full(coeffs, times, seg, 0.2, 5.0, 0.01, 1, want_times=wt,
                                                         capacity=ref.total)
        for g, w in ((got, want), (got_f, want_f)):
            for i, what in enumerate(("samples", "sample times", "counts", "offsets")):
                if w[i] is None:
                    assert g[i] is None
                else:
                    _same_bits("equal K, uniform " + what, g[i], w[i])


# ------------------------------------------------------------------ case 3
@pytest.mark.parametrize("D", [3, 2])
def test_window_edges_with_empty_neighbours(gpu_ctx, D):
    """t_start = 3.6 lies beyond the end of the short trajectories (K = 1, 2: at most 3 s; count 0, between
    non-empty ones, also first and last of the batch) and inside the long ones (K >= 6: at least 4.8 s);
    it is exactly the third vertex of trajectory 3, and t_end cuts trajectory 3 in its fifth segment."""
    Ks = [1, 6, 2, 7, 1, 9, 6, 2, 7, 1]
    cl, tl = _blocks(300 + D, Ks, D, 10, 0.8, 1.5)
    tl[3][:] = [1.2, 1.1, 1.3, 1.25, 1.15, 1.2, 1.3]
    ts = float(np.cumsum(tl[3])[2])
    te = ts + 1.77
    ref = _reference(cl, tl, ts, te, 0.01, 0)
    assert empties(tl, ts) == {0, 2, 4, 7, 9}
    runs = _runs(ref, 3, tl, ts, te, 0.01)
    assert runs[0][1] == 3 and ref.st[ref.offsets[3]] == ts and runs[-1][1] == 4 < Ks[3] - 1
    _check(gpu_ctx, "window", cl, tl, ts, te, 0.01, 0, ref=ref, device=D == 3, misaligned=True)


EDGES = ["dyadic_open", "dt_longer_than_segments", "ties_at_2p20", "start_on_vertex", "negative_start", "start_at_total"]


@pytest.mark.parametrize("name", EDGES)
@pytest.mark.parametrize("D", [3, 2])
def test_clock_edges_at_mixed_k(gpu_ctx, name, D):
    """The uniform suite's clock-edge inputs (CLOCK_EDGES: dyadic dt, dt > T_i, ties, t_start on a vertex,
    at the total, negative) at rows 1 and 5 of 7, between ordinary rows of other segment counts in the
    same clock wave.  Where t_start lies beyond the ordinary rows (ties_at_2p20) they are the empty
    neighbours."""
    special, scale, dt, ts, te, want_n, _, _ = CLOCK_EDGES[name]
    K = len(special)
    Ks = [2, K, K + 3, 1, 4, K, K + 1]
    cl, tl = _blocks(400 + len(name), Ks, D, 10, 0.5 * scale, 1.5 * scale)
    tl[1] = np.array(special, dtype=np.float64)
    tl[5] = np.array(special, dtype=np.float64)
    ref = _reference(cl, tl, ts, te, dt, 0)
    assert ref.counts[1] == ref.counts[5] and (want_n is None or ref.counts[1] == want_n)
    _check(gpu_ctx, name, cl, tl, ts, te, dt, 0, ref=ref, device=name == "dyadic_open")


# ------------------------------------------------------------------ case 4
@pytest.mark.parametrize("D", [2, 3])
def test_run_table_overflow_next_to_stored_clocks(gpu_ctx, D):
    """The uniform suite's K = 30, times in [1, 3], dt = 0.01 trajectory has more than 256 runs: the table
    overflows.  Next to it a K = 2 trajectory and a K = 30 one with short times, both stored whole.
    D = 2: eval_range_kernel<6, 0, 0, false> resumes the clock from RunHead on lane 0; D = 3: the
    stored-run launch takes rows 1 and 2 and the `rest` launch row 0."""
    N = 6
    cl, tl = _blocks(500 + D, [30, 2, 30], D, N, 1.0, 3.0)
    tl[2] *= 0.03
    ref = _reference(cl, tl, 0.0, T_END_OPEN, 0.01, 0)
    nr = [len(_runs(ref, b, tl, 0.0, T_END_OPEN, 0.01)) for b in range(3)]
    print("run-table overflow: runs %s, samples %s" % (nr, ref.counts))
    assert nr[0] > RUN_TABLE and 0 < nr[1] <= RUN_TABLE and 0 < ref.counts[2] < RUN_TABLE
    _check(gpu_ctx, "overflow D=%d" % D, cl, tl, 0.0, T_END_OPEN, 0.01, 0, ref=ref, device=True)


# ------------------------------------------------------------------ case 5
def _threshold_batch(K, seed):
    """[K_max (stored whole), K = 1, K_max (more than 256 runs: the rest launch), K = 5]: the shape of the
    uniform suite's stored-run case; the short trajectories' times are scaled so that they last 3 s and
    4 s longer than the shared t_start, the big ones' K - 10th vertex."""
    N, D = 10, 3
    cl, tl = _blocks(seed, [K, 1, K, 5], D, N, 0.5, 1.5)
    tl[2] = tl[0].copy()
    tl[2][:20] *= 12.0
    ts = float(np.cumsum(tl[0])[K - 11])
    tl[1] = np.array([ts + 3.0])
    tl[3] = tl[3] * ((ts + 4.0) / tl[3].sum())
    return cl, tl, ts


@pytest.mark.parametrize("K,kernel", [(229, "pc"), (230, "st"), (250, "st")])
def test_lds_thresholds_by_k_max(gpu_ctx, K, kernel):
    """D = 3, N = 10: K_max = 229 is the last of eval_range_pc_kernel, 230 the first and 250 the last of
    eval_range_kernel<10, 0, 3, true>; the K = 1 and K = 5 trajectories run in blocks whose LDS is sized
    for K_max."""
    N = 10
    assert (_lds_pc(N, K) <= LDS_MAX) == (kernel == "pc") and _lds(N, 3, K) <= LDS_MAX
    assert {"pc": _lds_pc(N, K + 1) > LDS_MAX, "st": _lds_pc(N, K - 1) <= LDS_MAX or _lds(N, 3, K + 1) > LDS_MAX}[kernel]
    cl, tl, ts = _threshold_batch(K, 600 + K)
    ref = _reference(cl, tl, ts, T_END_OPEN, 0.01, 0)
    runs = [_runs(ref, b, tl, ts, T_END_OPEN, 0.01) for b in range(4)]
    print("K_max=%d: samples %s, runs %s" % (K, ref.counts, [len(r) for r in runs]))
    assert 0 < len(runs[0]) <= RUN_TABLE and runs[0][0][1] == K - 10
    assert len(runs[2]) > RUN_TABLE and _segments_crossed(runs[2]) > 150
    assert 250 < ref.counts[1] < 450 and 250 < ref.counts[3] < 550 and len(runs[1]) <= RUN_TABLE >= len(runs[3])
    _check(gpu_ctx, "K_max=%d %s" % (K, kernel), cl, tl, ts, T_END_OPEN, 0.01, 0, ref=ref, device=True, misaligned=True)


def test_lds_limit_is_a_clean_error(gpu_ctx):
    """K_max = 251: the sample kernels' LDS does not fit.  The count call succeeds with the right counts;
    both sample calls return the uniform call's non-zero result with a message and write nothing; the
    context then serves an ordinary call."""
    from mav_trajectory_generation_cmake_amd.solver import _addr
    N, D, K = 10, 3, 251
    assert _lds(N, D, K) > LDS_MAX >= _lds(N, D, K - 1)
    cl, tl, ts = _threshold_batch(K, 651)
    cl, tl = cl[:2] + cl[3:], tl[:2] + tl[3:]  # (without the long-clock row: the counts are all this case needs)
    coeffs, times, seg = _csr(cl, tl)
    B = len(seg)
    O = _oracle()
    want = np.array([O.evaluate_range(c, t, ts, T_END_OPEN, 0.01, 0, max_samples=0)[2] for c, t in zip(cl, tl)],
                    dtype=np.int64)
    assert want.min() > 0
    lib, h = gpu_ctx._lib, gpu_ctx.handle
    gpu_ctx.reset_stream()
    counts = np.zeros(B, dtype=np.int64)
    rc = lib.mtg_evaluate_range_ragged_batch(h, N, D, B, _addr(seg), None, _addr(times), ts, T_END_OPEN, 0.01, 0,
                                             _addr(counts), None, None, None, 0)
    assert rc == 0
    _same_bits("K_max = 251 counts", counts, want)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    total = int(counts.sum())
    out, st = np.full((total, D), SENTINEL), np.full(total, SENTINEL)
    rc = lib.mtg_evaluate_range_ragged_batch(h, N, D, B, _addr(seg), _addr(coeffs), _addr(times), ts, T_END_OPEN, 0.01,
                                             0, _addr(counts), _addr(offsets), _addr(out), _addr(st), 0)
    msg = lib.mtg_last_error(h).decode()
    # the uniform call at K = K_max (on the K = 251 trajectory alone): the same result, the same kind of message
    c1 = np.zeros(1, dtype=np.int64)
    o1 = np.zeros(1, dtype=np.int64)
    out1 = np.full((int(want[0]), D), SENTINEL)
    c1[0] = want[0]
    rc_u = lib.mtg_evaluate_range_batch(h, N, D, K, 1, _addr(np.ascontiguousarray(cl[0])),
                                        _addr(np.ascontiguousarray(tl[0])), ts, T_END_OPEN, 0.01, 0, _addr(c1), _addr(o1),
                                        _addr(out1), None, 0)
    msg_u = lib.mtg_last_error(h).decode()
    # (the uniform call's message is the failed launch expression, cut at the message buffer's length; the
    # ragged call's names its check and ends with the HIP error's text)
    assert rc == rc_u != 0 and len(msg_u) > 0 and msg.endswith("invalid argument (1)")
    assert (out == SENTINEL).all() and (st == SENTINEL).all() and (out1 == SENTINEL).all()
    cnt2, off2, tot2 = np.full(B, -1, dtype=np.int64), np.full(B, -1, dtype=np.int64), np.full(1, -1, dtype=np.int64)
    rc = lib.mtg_evaluate_range_ragged_batch_full(h, N, D, B, _addr(seg), _addr(coeffs), _addr(times), ts, T_END_OPEN,
                                                  0.01, 0, _addr(cnt2), _addr(off2), _addr(tot2), _addr(out), _addr(st),
                                                  total, 0)
    assert rc == rc_u and (out == SENTINEL).all() and (st == SENTINEL).all()
    _same_bits("K_max = 251 counts after the error", counts, want)
    cl2, tl2 = _blocks(653, [5, 2, 7, 1], D, N, 0.5, 1.5)
    _check(gpu_ctx, "after the LDS error", cl2, tl2, 0.0, T_END_OPEN, 0.01, 0)


# ------------------------------------------------------------------ case 6
def test_clock_reads_times_from_global_memory(gpu_ctx):
    """B = 34, N = 6, D = 3, K_b = 260 except one each of 1, 3 and 300, times in [0.05, 0.15], t_start = 0.
    The 1 and the 3 are the second block: with them inside the first, its 7844 segments would fit the
    budget of 8192.  So the first 32-trajectory block has 8360 segments, and by the rule the whole launch
    is eval_count_kernel<false, true> / eval_runs_kernel<false, true>, the second block's two lane pairs
    next to 30 idle ones included."""
    Ks = [260] * 32 + [1, 3]
    Ks[17] = 300
    assert sum(Ks[:32]) > PAIR_TRAJ * CLOCK_LDS_K >= sum(Ks[32:]) and not clock_staged(Ks)
    assert _lds(6, 3, max(Ks)) <= LDS_MAX
    cl, tl = _blocks(700, Ks, 3, 6, 0.05, 0.15)
    ref = _reference(cl, tl, 0.0, T_END_OPEN, 0.01, 2)
    runs17 = _runs(ref, 17, tl, 0.0, T_END_OPEN, 0.01)
    assert len(runs17) > RUN_TABLE and _segments_crossed(runs17) > 256
    _check(gpu_ctx, "global clock", cl, tl, 0.0, T_END_OPEN, 0.01, 2, ref=ref, device=True)


@pytest.mark.parametrize("D", [3, 2])
def test_clock_stays_staged_with_k_above_256(gpu_ctx, D):
    """B = 5, K_b = 300, 1, 7, 260, 2: 570 segments in the one block, so the times are staged in LDS
    although two trajectories have more than 256 segments -- slots the uniform kernels never had: a lane
    pair's slot starts at seg_off[b] - seg_off[b0] and is K_b > 256 long."""
    Ks = [300, 1, 7, 260, 2]
    assert clock_staged(Ks) and max(Ks) > CLOCK_LDS_K and _lds(6, D, max(Ks)) <= LDS_MAX
    cl, tl = _blocks(710 + D, Ks, D, 6, 0.05, 0.15)
    ref = _reference(cl, tl, 0.0, T_END_OPEN, 0.01, 1)
    assert _segments_crossed(_runs(ref, 0, tl, 0.0, T_END_OPEN, 0.01)) > 256
    assert _segments_crossed(_runs(ref, 3, tl, 0.0, T_END_OPEN, 0.01)) > 256
    _check(gpu_ctx, "staged K > 256", cl, tl, 0.0, T_END_OPEN, 0.01, 1, ref=ref, device=True, misaligned=True)


# ------------------------------------------------------------------ case 7
def test_pipeline_from_the_ragged_solve(gpu_ctx):
    """solve_linear_ragged_batch on generator problems (N = 10, D = 3, K_b in 2..12, B = 64, shuffled,
    device-resident): its coeffs and the times tensor go straight into the one-call form; the samples
    equal the oracle's evaluate_range on those same coefficients."""
    import torch
    from _ragged_cases import order_of, per_k_batches, ragged_of
    counts = {K: (5 if K in (11, 12) else 6) for K in range(2, 13)}
    batches = per_k_batches(10, 3, counts, seed0=71)
    order = order_of(batches, "shuffled", seed=71)
    assert len(order) == 64
    values, mask, times, seg = ragged_of(batches, order)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (values, mask, times)]
    sol = gpu_ctx.solve_linear_ragged_batch(10, 4, dev[0], dev[1], dev[2], seg, status=True)
    assert sol["coeffs"].is_cuda and not sol["status"].cpu().numpy().any()
    dt = 0.05
    got = gpu_ctx.evaluate_range_ragged_batch_full(sol["coeffs"], dev[2], seg, 0.0, T_END_OPEN, dt, 0)
    torch.cuda.synchronize()
    assert got[0].is_cuda
    got = tuple(g.cpu().numpy() for g in got)
    cl = mtg.split_ragged(sol["coeffs"].cpu().numpy(), seg, "coeffs", D=3)
    tl = mtg.split_ragged(times, seg, "times")
    ref = _reference(cl, tl, 0.0, T_END_OPEN, dt, 0)
    _conditions(tl, 0.0, ref)
    _compare("pipeline", got, ref, True)
    gpu_ctx.reset_stream()


# ------------------------------------------------------------------ cases 8 and 9
@pytest.fixture(scope="module")
def small():
    Ks = [3, 1, 8, 2, 5, 13, 1, 4]
    cl, tl = _blocks(800, Ks, 3, 10, 0.3, 1.5)
    return dict(cl=cl, tl=tl, ref=_reference(cl, tl, 0.0, T_END_OPEN, 0.01, 0))


def test_one_call_protocol(gpu_ctx, small):
    """Capacity exactly total succeeds; total - 1 returns MTG_ERR_TOO_LARGE with counts, offsets and total
    filled and out untouched (host arrays and device pointers); with DEVICE_PTRS | ASYNC the call returns
    MTG_OK and the caller reads total itself."""
    import torch
    from mav_trajectory_generation_cmake_amd.solver import _addr
    ref = small["ref"]
    _conditions(small["tl"], 0.0, ref)
    coeffs, times, seg = _csr(small["cl"], small["tl"])
    B, D, N = len(seg), 3, 10
    lib, h = gpu_ctx._lib, gpu_ctx.handle
    gpu_ctx.reset_stream()

    def host_call(capacity):
        cnt, off, tot = np.full(B, -1, dtype=np.int64), np.full(B, -1, dtype=np.int64), np.full(1, -1, dtype=np.int64)
        out, st = np.full((ref.total, D), SENTINEL), np.full(ref.total, SENTINEL)
        rc = lib.mtg_evaluate_range_ragged_batch_full(h, N, D, B, _addr(seg), _addr(coeffs), _addr(times), 0.0,
                                                      T_END_OPEN, 0.01, 0, _addr(cnt), _addr(off), _addr(tot),
                                                      _addr(out), _addr(st), capacity, 0)
        return rc, cnt, off, tot, out, st

    rc, cnt, off, tot, out, st = host_call(ref.total)
    assert rc == 0 and tot[0] == ref.total
    _compare("capacity = total", (out, st, cnt, off), ref, True)
    rc, cnt, off, tot, out, st = host_call(ref.total - 1)
    assert rc == nat.MTG_ERR_TOO_LARGE and tot[0] == ref.total
    _same_bits("short capacity counts", cnt, ref.counts)
    _same_bits("short capacity offsets", off, ref.offsets)
    assert (out == SENTINEL).all() and (st == SENTINEL).all()

    c_d, t_d = torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda()
    gpu_ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for capacity, flags in ((ref.total - 1, nat.MTG_FLAG_DEVICE_PTRS),
                            (ref.total - 1, nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC),
                            (ref.total, nat.MTG_FLAG_DEVICE_PTRS | nat.MTG_FLAG_ASYNC)):
        cnt_d = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        off_d = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        tot_d = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        out_d = torch.full((ref.total, D), SENTINEL, dtype=torch.float64, device="cuda")
        st_d = torch.full((ref.total,), SENTINEL, dtype=torch.float64, device="cuda")
        rc = lib.mtg_evaluate_range_ragged_batch_full(h, N, D, B, _addr(seg), _addr(c_d), _addr(t_d), 0.0, T_END_OPEN,
                                                      0.01, 0, _addr(cnt_d), _addr(off_d), _addr(tot_d), _addr(out_d),
                                                      _addr(st_d), capacity, flags)
        torch.cuda.synchronize()
        asynchronous = bool(flags & nat.MTG_FLAG_ASYNC)
        assert rc == (0 if asynchronous or capacity >= ref.total else nat.MTG_ERR_TOO_LARGE)
        assert tot_d.item() == ref.total
        _same_bits("device counts", cnt_d.cpu().numpy(), ref.counts)
        _same_bits("device offsets", off_d.cpu().numpy(), ref.offsets)
        if capacity >= ref.total:
            _compare("device capacity = total", (out_d.cpu().numpy(), st_d.cpu().numpy(), cnt_d.cpu().numpy(),
                                                 off_d.cpu().numpy()), ref, True)
        else:
            assert (out_d == SENTINEL).all().item() and (st_d == SENTINEL).all().item()
    gpu_ctx.reset_stream()


def test_two_async_calls_with_different_seg_count(gpu_ctx, small, mixed):
    """Back to back on one context, no synchronisation between them: the second call's segment offsets
    must not overwrite those the first call's kernels still read."""
    import torch
    calls = []
    for src, lo, hi in ((mixed, 0, 65), (small, 0, 8), (mixed, 20, 50)):
        cl, tl = src["cl"][lo:hi], src["tl"][lo:hi]
        D = cl[0].shape[1]
        coeffs, times, seg = _csr(cl, tl)
        calls.append((src["ref"].head(lo, hi, D), seg, torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda()))
    torch.cuda.synchronize()
    outs = [gpu_ctx.evaluate_range_ragged_batch_full(c_d, t_d, seg, 0.0, T_END_OPEN, 0.01, 0, capacity=ref.total,
                                                     asynchronous=True) for ref, seg, c_d, t_d in calls]
    torch.cuda.synchronize()
    for i, ((ref, _, _, _), (out, st, cnt, off, tot)) in enumerate(zip(calls, outs)):
        assert tot.item() == ref.total
        _compare("async call %d" % i, (out.cpu().numpy()[:ref.total], st.cpu().numpy()[:ref.total], cnt.cpu().numpy(),
                                       off.cpu().numpy()), ref, True)
    gpu_ctx.reset_stream()


# ------------------------------------------------------------------ case 10
def test_argument_errors_and_the_empty_batch(gpu_ctx, small):
    from mav_trajectory_generation_cmake_amd.solver import _addr
    coeffs, times, seg = _csr(small["cl"], small["tl"])
    B, D, N = len(seg), 3, 10
    lib, h = gpu_ctx._lib, gpu_ctx.handle
    gpu_ctx.reset_stream()
    cnt, off, tot = np.full(B, -7, dtype=np.int64), np.zeros(B, dtype=np.int64), np.full(1, -7, dtype=np.int64)
    out, st = np.full((16, D), SENTINEL), np.full(16, SENTINEL)

    def two(N=N, D=D, B=B, seg=seg, dt=0.01, der=0, times=times, counts=cnt):
        return lib.mtg_evaluate_range_ragged_batch(h, N, D, B, _addr(seg), _addr(coeffs), _addr(times), 0.0, 1.0, dt, der,
                                                   _addr(counts), _addr(off), _addr(out), _addr(st), 0)

    def one(N=N, D=D, B=B, seg=seg, dt=0.01, der=0, capacity=16, total=tot):
        return lib.mtg_evaluate_range_ragged_batch_full(h, N, D, B, _addr(seg), _addr(coeffs), _addr(times), 0.0, 1.0, dt,
                                                        der, _addr(cnt), _addr(off), _addr(total), _addr(out), _addr(st),
                                                        capacity, 0)

    bad = seg.copy()
    bad[3] = 0
    for f in (two, one):
        assert f(N=5) == nat.MTG_ERR_UNSUPPORTED_N
        assert f(D=0) == nat.MTG_ERR_SIZE_MISMATCH
        assert f(B=-1) == nat.MTG_ERR_SIZE_MISMATCH
        assert f(dt=0.0) == nat.MTG_ERR_INVALID_ARGUMENT
        assert f(dt=float("nan")) == nat.MTG_ERR_INVALID_ARGUMENT
        assert f(der=-1) == nat.MTG_ERR_INVALID_ARGUMENT
        assert f(seg=None) == nat.MTG_ERR_INVALID_ARGUMENT
        assert f(seg=bad) == nat.MTG_ERR_SIZE_MISMATCH
        assert len(lib.mtg_last_error(h).decode()) > 0
        assert f(B=0) == nat.MTG_OK
    assert one(capacity=-1) == nat.MTG_ERR_SIZE_MISMATCH
    assert two(times=None) == nat.MTG_ERR_INVALID_ARGUMENT
    assert two(counts=None) == nat.MTG_ERR_INVALID_ARGUMENT
    assert one(total=None) == nat.MTG_ERR_INVALID_ARGUMENT
    assert tot[0] == 0  # (the one-call form with batch = 0 sets the total)
    assert (cnt == -7).all() and (out == SENTINEL).all() and (st == SENTINEL).all()
    assert lib.mtg_evaluate_range_ragged_batch(None, N, D, B, _addr(seg), None, _addr(times), 0.0, 1.0, 0.01, 0, _addr(cnt),
                                               None, None, None, 0) == nat.MTG_ERR_INVALID_ARGUMENT
    # and the context still serves a call
    _check(gpu_ctx, "after the errors", small["cl"], small["tl"], 0.0, T_END_OPEN, 0.01, 0, ref=small["ref"])
