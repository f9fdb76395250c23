"""mtg_evaluate_range_batch / mtg_evaluate_range_batch_full (csrc/mtg_eval.hip) against the sequential
restatement of Trajectory::evaluateRange (oracle.pyoracle.evaluate_range), bit for bit: counts, offsets,
every sample row and every sample time of every trajectory, through the two-call and the one-call API,
with and without sample times, on every kernel the host chooses between:

  group 1  every N instantiation, the derivative's compile-time / run-time / all-zero variants, and
           eval_range_kernel<N, DER, 0, false> as the only sample kernel (D != 3)
  group 2  the clock's edges (Clock / PairClock: dyadic dt, dt > T_i, t_start on vertices, ties, tiny times)
  group 3  one PairClock wave whose 32 lane pairs stop at very different times
  group 4  a run table that overflows off the D = 3 path: the clock resumed from RunHead on lane 0
  group 5  eval_range_kernel<N, DER, 3, true> (the one-wave stored-run kernel), its neighbour
           eval_range_pc_kernel, the `rest` launch next to each, and the clean error past the LDS limit
  group 6  eval_count_kernel<false> / eval_runs_kernel<false> (K > 256: segment times from global memory)

Coefficients are seeded normal draws [B][K][D][N], not solves, so N, D and K vary freely; a few
trajectories carry an all-zero segment and a -0.0 entry.  The reference's quirk is kept by both sides:
sample times count from the start of the segment that holds t_start and the loop stops when that clock
reaches t_end (times [0.7, 1.3, 0.9], t_start = t_end = 1.0, dt = 0.01: 30 samples, not 0).

Which kernel a case reaches depends on its number of runs (the kernels' unit of work: a stretch of
samples on which tin and acc both step by a constant number of ulps inside one binade and one segment).
_model_runs restates Clock::next's run splitting with exact integers; it is used only to assert, on the
CPU, that each case's inputs reach the path they are there for, and is itself checked against the
oracle's sample count and sample times."""
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_END_OPEN = 1e9  # "until the trajectory ends"
SENTINEL = 7.25

# launch_eval_range / eval_workspace_bytes (csrc/mtg_eval.hip).  Revisit these and groups 5 / 6 if kSpl,
# PcSlot, RunLds, kClockLdsK or the table's 256 runs change.
K_SPL, EVAL_THREADS = 2, 64
RUN_LDS = 32 * (5 * 8 + 2 * 8 + 4 * 4)                                    # sizeof(RunLds) = 2304
PC_SLOT = 8 * K_SPL * EVAL_THREADS * 3 + 8 * K_SPL * EVAL_THREADS + 16    # sizeof(PcSlot) = 4112
LDS_MAX = 64 * 1024
RUN_TABLE = 256   # runs per trajectory in the table (cap, below ~1.2e5 trajectories)
CLOCK_LDS_K = 256  # kClockLdsK: above it the clock kernels read the segment times from global memory


def _lds(N, D, K):
    """launch_eval_range's `lds`: the one-wave kernels' dynamic LDS; above 64 KiB the call fails."""
    return RUN_LDS + 8 * (K * D * N + (K_SPL if D == 3 else 1) * EVAL_THREADS * D)


def _lds_pc(N, K):
    """launch_eval_range's `lds_pc`: the producer / consumer kernel's LDS; above 64 KiB the D = 3
    stored-run launch is eval_range_kernel<N, DER, 3, true> instead."""
    return RUN_LDS + 8 * K * 3 * N + 2 * PC_SLOT


def _oracle():
    from oracle import pyoracle
    return pyoracle


# ------------------------------------------------------------------ inputs
def _coeffs(seed, B, K, D, N):
    """Seeded normal coefficients [B][K][D][N]; every third trajectory has one all-zero segment and
    one -0.0 entry in another."""
    c = np.random.default_rng(seed).standard_normal((B, K, D, N))
    for b in range(0, B, 3):
        c[b, b % K] = 0.0
        c[b, (b + 1) % K, b % D, b % N] = -0.0
    return c


def _uniform(seed, shape, lo, hi):
    return np.random.default_rng(seed).uniform(lo, hi, shape)


# ------------------------------------------------------------------ the truth
class _Ref:
    def __init__(self, rows, D):
        self.rows = rows
        self.counts = np.array([len(st) for _, st in rows], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)[:-1]]).astype(np.int64)
        self.total = int(self.counts.sum())
        self.out = np.concatenate([o for o, _ in rows]).reshape(self.total, D)
        self.st = np.concatenate([s for _, s in rows]).reshape(self.total)

    def head(self, lo, hi, D):
        return _Ref(self.rows[lo:hi], D)


def _reference(coeffs, times, ts, te, dt, der):
    """The oracle on every trajectory of the batch."""
    O = _oracle()
    rows = []
    for b in range(coeffs.shape[0]):
        n = O.evaluate_range(coeffs[b], times[b], ts, te, dt, der, max_samples=0)[2]
        assert 0 <= n <= 200000, "a case of this module never has this many samples: %d" % n
        out, st, n2 = O.evaluate_range(coeffs[b], times[b], ts, te, dt, der, max_samples=max(n, 1))
        assert n2 == n
        rows.append((out[:n].copy(), st[:n].copy()))
    return _Ref(rows, coeffs.shape[2])


def _same_bits(what, got, want, ref=None):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero((got.view(np.int64) != want.view(np.int64)).reshape(len(got), -1).any(axis=1)
                         if got.size else np.zeros(0, bool))
    if len(bad):
        i = int(bad[0])
        b = int(np.searchsorted(ref.offsets, i, side="right") - 1) if ref is not None and got.dtype != np.int64 else i
        at = " (trajectory %d, its sample %d)" % (b, i - int(ref.offsets[b])) if ref is not None else ""
        raise AssertionError("%s: %d of %d rows differ, first at %d%s: got %r, want %r"
                             % (what, len(bad), len(got), i, at, got[i], want[i]))


def _compare(what, got, ref, want_times):
    out, st, counts, offsets = got
    _same_bits(what + " counts", np.asarray(counts), ref.counts)
    _same_bits(what + " offsets", np.asarray(offsets), ref.offsets)
    _same_bits(what + " samples", np.asarray(out), ref.out, ref)
    if want_times:
        _same_bits(what + " sample times", np.asarray(st), ref.st, ref)
    else:
        assert st is None


def _check(ctx, name, coeffs, times, ts, te, dt, der=0, ref=None, device=False, misaligned=False):
    """Every API against the oracle, all trajectories: the two-call API and the one-call API from numpy
    arrays, each with and without sample times; device=True: the one-call API from device tensors as
    well; misaligned=True: the two-call API's sample call into an output that is only 8-B aligned."""
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    B, K, D, N = coeffs.shape
    if ref is None:
        ref = _reference(coeffs, times, ts, te, dt, der)
    t0 = time.perf_counter()
    for wt in (True, False):
        got = ctx.evaluate_range_batch(coeffs, times, ts, te, dt, der, want_times=wt)
        _compare("%s two-call%s" % (name, "" if wt else " no times"), got, ref, wt)
        got = ctx.evaluate_range_batch_full(coeffs, times, ts, te, dt, der, want_times=wt, capacity=ref.total)
        _compare("%s one-call%s" % (name, "" if wt else " no times"), got, ref, wt)
    if device or misaligned:
        import torch
        from mav_trajectory_generation_cmake_amd import _native as nat
        from mav_trajectory_generation_cmake_amd.solver import _addr
        c_d, t_d = torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda()
    if device:
        for wt in (True, False):
            got = ctx.evaluate_range_batch_full(c_d, t_d, ts, te, dt, der, want_times=wt, capacity=ref.total)
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
            nat.check(ctx._lib.mtg_evaluate_range_batch(ctx.handle, N, D, K, B, _addr(c_d), _addr(t_d), float(ts),
                                                        float(te), float(dt), int(der), _addr(cnt_d), _addr(off_d),
                                                        _addr(view), _addr(st_d) if wt else None,
                                                        nat.MTG_FLAG_DEVICE_PTRS), ctx.handle)
            torch.cuda.synchronize()
            assert buf[0].item() == SENTINEL and buf[-1].item() == SENTINEL
            _same_bits(name + " 8-B aligned samples", view.cpu().numpy().reshape(ref.total, D), ref.out, ref)
            if wt:
                assert st_d[-1].item() == SENTINEL
                _same_bits(name + " 8-B aligned sample times", st_d[:-1].cpu().numpy(), ref.st, ref)
    print("evaluateRange %s: N=%d D=%d K=%d B=%d derivative=%d total=%d samples, device calls %.3f s"
          % (name, N, D, K, B, der, ref.total, time.perf_counter() - t0))
    return ref


# ------------------------------------------------------------------ the run model (path conditions only)
def _ldexp(x, e):
    try:
        return math.ldexp(x, e)
    except OverflowError:
        return math.inf


def _progression(x, dt):
    """mtg_eval.hip progression(): (m, inc, E) with fl(x + dt) = (m + inc) 2^E while x stays in its binade."""
    if not (x > 0.0) or x < 2.2250738585072014e-308 or math.isinf(x):
        return None
    fr, e = math.frexp(x)
    m, E = int(math.ldexp(fr, 53)), e - 53
    f = _ldexp(dt, -E)
    if not f < float(2 ** 53 - m):
        return None
    q = math.floor(f)
    phi = f - q
    if phi < 0.5:
        inc = q
    elif phi > 0.5:
        inc = q + 1
    else:
        if m & 1:
            return None
        inc = q + (q & 1)
    return (m, inc, E) if inc > 0 else None


def _len_le(p, lim_scaled):
    if not lim_scaled < 4.0e18:
        return 1 << 62
    lim = int(lim_scaled)
    return 0 if lim < p[0] else (lim - p[0]) // p[1] + 1


def _model_runs(times, ts, te, dt):
    """Clock::init / next / settle of mtg_eval.hip with exact integer division: the runs of one
    trajectory as (n0, segment, single, acc0), and the sample count."""
    K = len(times)
    a, i = 0.0, 0
    for i in range(K):
        a += times[i]
        if a > ts:
            break
    if ts > a:
        return [], 0
    a -= times[i]
    seg, acc, tin, n, runs = i, a, ts - a, 0, []

    def settle(seg, acc, tin):
        if not acc < te:
            return seg, tin, True
        while tin > times[seg]:
            tin = tin - times[seg]
            seg += 1
            if seg >= K:
                return seg, tin, True
        return seg, tin, False

    seg, tin, done = settle(seg, acc, tin)
    while not done:
        pt, pa = _progression(tin, dt), _progression(acc, dt)
        L, single = 1, True
        if pt and pa:
            lim = min((2 ** 53 - 1 - pt[0]) // pt[1] + 1, (2 ** 53 - 1 - pa[0]) // pa[1] + 1,
                      _len_le(pt, _ldexp(float(times[seg]), -pt[2])))
            q = _ldexp(te, -pa[2])
            if q < 4.0e18:
                lim = min(lim, _len_le(pa, math.ceil(q) - 1.0))
            L, single = max(lim, 1), False
        runs.append((n, seg, single, acc))
        if L > 1:
            tin = math.ldexp(float(pt[0] + (L - 1) * pt[1]), pt[2])
            acc = math.ldexp(float(pa[0] + (L - 1) * pa[1]), pa[2])
        n += L
        tin += dt
        acc += dt
        seg, tin, done = settle(seg, acc, tin)
    return runs, n


def _runs(ref, b, times, ts, te, dt):
    """The model's runs of trajectory b, after checking the model against the oracle: the same sample
    count, and every run starts at the oracle's sample time."""
    runs, n = _model_runs([float(t) for t in times[b]], float(ts), float(te), float(dt))
    st = ref.rows[b][1]
    assert n == len(st), (b, n, len(st))
    for n0, _, _, acc0 in runs:
        assert np.float64(acc0).view(np.int64) == st[n0].view(np.int64), (b, n0)
    return runs


def _segments_crossed(runs):
    return runs[-1][1] - runs[0][1] if runs else 0


# ------------------------------------------------------------------ group 1
SHAPES = {(2, 1): (0, 1, 2, 5), (4, 2): (3, 4), (6, 3): (0, 3, 5, 6), (8, 4): (0, 7), (12, 5): (4, 5, 11, 12),
          (10, 1): (0, 9), (12, 3): (4, 5, 11, 12), (2, 3): (0, 1, 2, 5)}


@pytest.mark.parametrize("N,D", sorted(SHAPES))
def test_shapes_and_instantiations(gpu_ctx, N, D):
    """Every N instantiation of the sample kernels; DER at compile time (0..4), at run time (>= 5) and
    derivative >= N (all rows +0.0; N = 4 with the compile-time DER = 4).  D != 3: the run-time-D
    eval_range_kernel<N, DER, 0, false> is the only sample kernel (run table, no resume: a few tens of
    runs); D = 3: eval_range_pc_kernel<N, DER>.  B = 33 is one full clock wave and one with a single
    lane pair; K = 5, times in [0.5, 1.5], dt = 0.01, the whole trajectory."""
    B, K = 33, 5
    coeffs = _coeffs(100 + 16 * N + D, B, K, D, N)
    times = _uniform(200 + 16 * N + D, (B, K), 0.5, 1.5)
    assert _lds(N, D, K) <= LDS_MAX and _lds_pc(N, K) <= LDS_MAX
    for der in SHAPES[(N, D)]:
        ref = _check(gpu_ctx, "shapes", coeffs, times, 0.0, T_END_OPEN, 0.01, der, device=der == SHAPES[(N, D)][0])
        assert ref.counts.min() > 250
        if der >= N:  # exactly +0.0 on both sides (the comparison above is bitwise)
            assert not ref.out.view(np.int64).any()
        else:
            assert np.count_nonzero(ref.out) > 0.9 * ref.out.size
    assert max(len(_runs(ref, b, times, 0.0, T_END_OPEN, 0.01)) for b in range(B)) <= RUN_TABLE


# ------------------------------------------------------------------ group 2
def _edge_batch(special, scale, seed, N=10, D=3):
    """`special` at rows 1 and 5 of 7, ordinary rows (scale * [0.5, 1.5]) around them."""
    K = len(special)
    times = scale * _uniform(seed, (7, K), 0.5, 1.5)
    times[1] = times[5] = special
    return _coeffs(seed + 1, 7, K, D, N), times


T3 = [0.7, 1.3, 0.9]
T3_TOTAL = (0.7 + 1.3) + 0.9
P20 = 2.0 ** 20

# name: (times, ordinary rows' scale, dt, t_start, t_end, samples, runs, single runs) -- None: not stated
CLOCK_EDGES = {
    "dyadic_open": ([1, 0.5, 2, 0.25, 1], 1.0, 0.125, 0.0, T_END_OPEN, 39, 19, None),
    "dyadic_t_end_on_a_sample": ([1, 0.5, 2, 0.25, 1], 1.0, 0.125, 0.0, 1.0, 8, None, None),
    "dt_longer_than_segments": ([0.05, 0.07, 0.3, 0.02, 0.11, 0.4], 0.15, 0.25, 0.0, T_END_OPEN, 4, 4, 4),
    "start_on_vertex": (T3, 1.0, 0.01, 0.7 + 1.3, T_END_OPEN, None, None, None),
    "start_at_total": (T3, 1.0, 0.01, T3_TOTAL, T_END_OPEN, 1, None, None),
    "start_past_total": (T3, 1.0, 0.01, float(np.nextafter(T3_TOTAL, np.inf)), T_END_OPEN, 0, None, None),
    "negative_start": (T3, 1.0, 0.01, -0.3, T_END_OPEN, 320, 58, 40),
    "end_before_start": (T3, 1.0, 0.01, 1.0, 0.9, None, None, None),
    "end_at_start": (T3, 1.0, 0.01, 1.0, 1.0, 30, None, None),
    "end_one_ulp_after_start": (T3, 1.0, 0.01, 1.0, float(np.nextafter(1.0, np.inf)), None, None, None),
    "dt_one_third": (T3, 1.0, 1.0 / 3.0, 0.1, T_END_OPEN, None, None, None),
    # dt / ulp(acc) = 1.5 (then 1.25): every acc step is a round-to-even tie.  Never a dt at or below
    # half an ulp of acc, nor a t_start inside a 2^20-long segment: the reference loop would not end.
    "ties_at_2p20": ([P20] * 3, 1.0, 3 * 2.0 ** -33, P20, P20 + 2000 * 3 * 2.0 ** -33, 1500, 13, None),
    "ties_at_2p21": ([P20] * 3, 1.0, 5 * 2.0 ** -34, 2 * P20, 2 * P20 + 3000 * 5 * 2.0 ** -34, 1875, None, None),
    "tiny_dyadic": ([2.0 ** -20] * 3, 2.0 ** -20, 2.0 ** -27, 0.0, T_END_OPEN, 385, None, None),
    "tiny": ([1.3 * 2.0 ** -20, 0.7 * 2.0 ** -20, 2.0 ** -20], 2.0 ** -20, 1.1 * 2.0 ** -27, 0.0, T_END_OPEN, 350,
             None, None),
}


@pytest.mark.parametrize("name", sorted(CLOCK_EDGES))
@pytest.mark.parametrize("D", [3, 2])
def test_clock_edges(gpu_ctx, name, D):
    """Clock / PairClock at their edges, the special times next to ordinary rows in one clock wave:
    samples exactly on T_i (included) and on t_end (excluded), several segment switches in one
    settle(), t_start on a vertex / the total / past it / negative (single steps until tin > 0),
    t_end <= t_start (the reference's clock starts at the segment's start, so it still samples),
    round-to-even ties at every step, and binade crossings at every few steps from acc = 0.
    D = 3: eval_range_pc_kernel; D = 2: eval_range_kernel<10, 0, 0, false>."""
    special, scale, dt, ts, te, want_n, want_runs, want_single = CLOCK_EDGES[name]
    coeffs, times = _edge_batch(special, scale, 300 + len(name), D=D)
    ref = _reference(coeffs, times, ts, te, dt, 0)
    runs = _runs(ref, 1, times, ts, te, dt)
    print("%s: %d samples in %d runs, %d single" % (name, ref.counts[1], len(runs), sum(r[2] for r in runs)))
    assert ref.counts[1] == ref.counts[5]
    if want_n is not None:
        assert ref.counts[1] == want_n
    if want_runs is not None:
        assert len(runs) == want_runs
    if want_single is not None:
        assert sum(r[2] for r in runs) == want_single
    _check(gpu_ctx, name, coeffs, times, ts, te, dt, 0, ref=ref, device=name in ("dyadic_open", "negative_start"))


# ------------------------------------------------------------------ group 3
def _heterogeneous_times(B=65, K=6):
    """Rows cycle through five kinds, so adjacent lane pairs differ in kind: tiny times (the total far
    below t_start = 0.4: no samples), ordinary, 20 times longer, dyadic, short ([0.05, 0.1]); row 63,
    the last of the second 32-row block, is tiny as well (between a long and a short row).  The calls
    stop at t_end = 50, inside the long rows, which keeps a call under 1e5 samples."""
    u = _uniform(401, (B, K), 0.5, 1.5)
    times = np.empty((B, K))
    dyadic = np.array([1, 0.5, 2, 0.25, 1, 0.5])
    for b in range(B):
        kind = 0 if b == 63 else b % 5
        times[b] = [u[b] * 2.0 ** -20, u[b], 20.0 * u[b], np.roll(dyadic, b), 0.05 + 0.05 * (u[b] - 0.5)][kind]
    return times


@pytest.fixture(scope="module", params=[3, 2])
def heterogeneous(request):
    D = request.param
    times = _heterogeneous_times()
    coeffs = _coeffs(402 + D, 65, 6, D, 10)
    ts, te, dt = 0.4, 50.0, 0.01
    ref = _reference(coeffs, times, ts, te, dt, 1)
    return dict(D=D, times=times, coeffs=coeffs, ts=ts, te=te, dt=dt, ref=ref)


def test_heterogeneous_wave_inputs(heterogeneous):
    """The condition on the inputs, from the oracle: lane pairs with no samples at all (done from
    init) sit between pairs with hundreds or thousands of samples, at the first row of a 32-row block
    (0), the last (63) and inside (5, 10, ...), and the longest clocks have tens of runs."""
    h = heterogeneous
    c = h["ref"].counts
    assert c[0] == 0 and c[1] > 300
    assert c[63] == 0 and c[62] > 3000 and c[64] > 0
    assert all(c[b] == 0 and c[b + 1] > 300 for b in range(5, 60, 5))
    assert np.count_nonzero(c[4::5]) >= 10 and c[4::5].max() < 20  # the short rows: a handful of samples
    assert c[31] > 300 and c[32] > 3000
    nr = [len(_runs(h["ref"], b, h["times"], h["ts"], h["te"], h["dt"])) for b in range(65)]
    assert nr[0] == 0 and min(nr[b] for b in range(2, 65, 5)) > 30 and max(nr) <= RUN_TABLE
    print("heterogeneous: counts min %d max %d total %d, runs max %d" % (c.min(), c.max(), c.sum(), max(nr)))


@pytest.mark.parametrize("lo,hi", [(0, 65), (0, 1), (1, 2), (0, 31), (0, 32)])
def test_heterogeneous_wave(gpu_ctx, heterogeneous, lo, hi):
    """PairClock's DPP pair_swap under divergent control flow: in eval_count_kernel and
    eval_runs_kernel, the 32 lane pairs of a wave leave the clock loop after 0 to ~60 runs.  B = 65
    (two full waves and one pair), and 1 (a trajectory without and one with samples), 31, 32.
    D = 3: eval_range_pc_kernel; D = 2: eval_range_kernel<10, 1, 0, false>."""
    h = heterogeneous
    _check(gpu_ctx, "heterogeneous[%d:%d]" % (lo, hi), h["coeffs"][lo:hi], h["times"][lo:hi], h["ts"], h["te"],
           h["dt"], 1, ref=h["ref"].head(lo, hi, h["D"]), device=(lo, hi) == (0, 65))


# ------------------------------------------------------------------ group 4
def test_run_table_overflow_run_time_d(gpu_ctx):
    """N = 6, D = 2, K = 30, times in [1, 3], dt = 0.01: 277 runs, more than the table's 256, so
    eval_range_kernel<6, 0, 0, false> takes 256 runs from the table and resumes the clock from
    RunHead on lane 0; one row with short times (under 256 samples, so under 256 runs) ends inside
    the table."""
    N, D, K, B = 6, 2, 30, 3
    times = _uniform(501, (B, K), 1.0, 3.0)
    times[1] *= 0.03
    coeffs = _coeffs(502, B, K, D, N)
    ref = _reference(coeffs, times, 0.0, T_END_OPEN, 0.01, 0)
    nr = [len(_runs(ref, b, times, 0.0, T_END_OPEN, 0.01)) for b in range(B)]
    print("run-table overflow: runs %s, samples %s" % (nr, ref.counts))
    assert nr[0] > RUN_TABLE and nr[2] > RUN_TABLE and 0 < ref.counts[1] < RUN_TABLE
    _check(gpu_ctx, "overflow D=2", coeffs, times, 0.0, T_END_OPEN, 0.01, 0, ref=ref, device=True)


# ------------------------------------------------------------------ group 5
# D = 3: lds_pc = 2304 + 24 K N + 2 * 4112 <= 65536  <=>  K N <= 2292: N = 10: K <= 229, N = 12: K <= 191
#        (eval_range_pc_kernel); above it eval_range_kernel<N, DER, 3, true> while
#        lds = 2304 + 24 K N + 8 * 2 * 64 * 3 <= 65536  <=>  K N <= 2506: N = 10: K <= 250, N = 12: K <= 208;
#        above that the sample call fails.
STORED_RUN_CASES = [(10, 229, "pc"), (10, 230, "st"), (10, 250, "st"), (12, 191, "pc"), (12, 192, "st"),
                    (12, 208, "st")]


@pytest.mark.parametrize("N,K,kernel", STORED_RUN_CASES)
def test_one_wave_stored_run_kernel_and_neighbours(gpu_ctx, N, K, kernel):
    """Both sides of lds_pc = 64 KiB and the last K below lds = 64 KiB, D = 3.  Row 0 starts at its
    K - 10th vertex (its whole clock, under 256 runs, is stored: the stored-run launch); row 1 has
    all times halved (no samples); row 2's first 20 segments are 12 times longer, so t_start falls
    early and its clock has more than 256 runs over more than 150 segments (K itself is below 256):
    the second launch, eval_range_kernel<N, 0, 0, false> with `rest`, resumed from RunHead.  Aligned
    outputs, and an output that is only 8-B aligned."""
    assert (_lds_pc(N, K) <= LDS_MAX) == (kernel == "pc") and _lds(N, 3, K) <= LDS_MAX
    # K sits on a threshold: the last K of the producer / consumer kernel, the first or the last of the other
    at_edge = {"pc": _lds_pc(N, K + 1) > LDS_MAX, "st": _lds_pc(N, K - 1) <= LDS_MAX or _lds(N, 3, K + 1) > LDS_MAX}
    assert at_edge[kernel]
    times = np.repeat(_uniform(600 + K, (1, K), 0.5, 1.5), 3, axis=0)
    times[1] *= 0.5
    times[2, :20] *= 12.0
    coeffs = _coeffs(601 + K, 3, K, 3, N)
    ts = float(np.cumsum(times[0])[K - 11])  # the left-to-right sum of the first K - 10 segment times
    ref = _reference(coeffs, times, ts, T_END_OPEN, 0.01, 0)
    runs = [_runs(ref, b, times, ts, T_END_OPEN, 0.01) for b in range(3)]
    print("stored-run N=%d K=%d: samples %s, runs %s, row 2 crosses %d segments"
          % (N, K, ref.counts, [len(r) for r in runs], _segments_crossed(runs[2])))
    assert 800 < ref.counts[0] < 1300 and 0 < len(runs[0]) <= RUN_TABLE and runs[0][0][1] == K - 10
    assert ref.counts[1] == 0
    assert len(runs[2]) > RUN_TABLE and _segments_crossed(runs[2]) > 150
    _check(gpu_ctx, "stored-run " + kernel, coeffs, times, ts, T_END_OPEN, 0.01, 0, ref=ref, device=True,
           misaligned=True)


def test_lds_limit_is_a_clean_error(gpu_ctx):
    """N = 10, D = 3, K = 251: lds > 64 KiB.  The count call succeeds; the sample call returns a
    non-zero status with a message, before any sample kernel is launched, and writes nothing; the
    context then serves an ordinary call."""
    from mav_trajectory_generation_cmake_amd.solver import _addr
    N, D, K, B = 10, 3, 251, 2
    assert _lds(N, D, K) > LDS_MAX >= _lds(N, D, K - 1)
    times = _uniform(650, (B, K), 0.5, 1.5)
    coeffs = _coeffs(651, B, K, D, N)
    O = _oracle()
    want = np.array([O.evaluate_range(coeffs[b], times[b], 0.0, T_END_OPEN, 0.01, 0, max_samples=0)[2]
                     for b in range(B)], dtype=np.int64)
    lib, h = gpu_ctx._lib, gpu_ctx.handle
    gpu_ctx.reset_stream()
    counts = np.zeros(B, dtype=np.int64)
    rc = lib.mtg_evaluate_range_batch(h, N, D, K, B, None, _addr(times), 0.0, T_END_OPEN, 0.01, 0, _addr(counts),
                                      None, None, None, 0)
    assert rc == 0
    _same_bits("K = 251 counts", counts, want)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    total = int(counts.sum())
    out = np.full((total, D), SENTINEL)
    st = np.full(total, SENTINEL)
    rc = lib.mtg_evaluate_range_batch(h, N, D, K, B, _addr(coeffs), _addr(times), 0.0, T_END_OPEN, 0.01, 0,
                                      _addr(counts), _addr(offsets), _addr(out), _addr(st), 0)
    assert rc != 0
    assert len(lib.mtg_last_error(h).decode()) > 0
    assert (out == SENTINEL).all() and (st == SENTINEL).all()
    _same_bits("K = 251 counts after the error", counts, want)
    small = _uniform(652, (4, 5), 0.5, 1.5)
    _check(gpu_ctx, "after the LDS error", _coeffs(653, 4, 5, D, N), small, 0.0, T_END_OPEN, 0.01, 0)


# ------------------------------------------------------------------ group 6
@pytest.mark.parametrize("N,D,K", [(6, 3, 260), (4, 2, 300)])
@pytest.mark.parametrize("start", ["whole", "tail"])
def test_more_segments_than_the_clock_stages(gpu_ctx, N, D, K, start):
    """K > 256 = kClockLdsK: eval_count_kernel<false> / eval_runs_kernel<false>, the segment times
    read from global memory inside the clock loop.  Times in [0.05, 0.15], dt = 0.01, B = 34.
    whole: t_start = 0, every row crosses more than 256 segments in about 1200 runs (the table
    overflows: lane 0 resumes; D = 3: the `rest` launch).  tail: t_start at row 0's 12th-last
    vertex, every clock is stored whole (D = 3: eval_range_pc_kernel)."""
    B = 34
    assert K > CLOCK_LDS_K and _lds(N, D, K) <= LDS_MAX and _lds_pc(N, K) <= LDS_MAX
    times = _uniform(700 + K, (B, K), 0.05, 0.15)
    coeffs = _coeffs(701 + K, B, K, D, N)
    ts = 0.0 if start == "whole" else float(np.cumsum(times[0])[K - 13])
    ref = _reference(coeffs, times, ts, T_END_OPEN, 0.01, 2)
    runs = [_runs(ref, b, times, ts, T_END_OPEN, 0.01) for b in range(B)]
    nr = [len(r) for r in runs]
    print("K=%d %s: samples %d..%d, runs %d..%d" % (K, start, ref.counts.min(), ref.counts.max(), min(nr), max(nr)))
    if start == "whole":
        assert ref.counts.min() > 2000 and min(nr) > 4 * RUN_TABLE  # (about 1200 runs; the table holds 256)
        assert min(_segments_crossed(r) for r in runs) > 256
    else:
        assert runs[0][0][1] == K - 12 and 80 < ref.counts[0] < 180
        assert max(nr) <= RUN_TABLE and np.count_nonzero(ref.counts) >= B - 2
    _check(gpu_ctx, "K=%d %s" % (K, start), coeffs, times, ts, T_END_OPEN, 0.01, 2, ref=ref, device=True)
