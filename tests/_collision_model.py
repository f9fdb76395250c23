"""Stand-in for the reference's collision term, written from
polynomial_optimization_nonlinear_impl.h: getCostAndGradientCollision (:1523-1709),
getCostAndGradientPotentialESDF (:1713-1806), getDistanceSDF with lerp / triLerp (:1846-1904,
:2436-2464) and getCostPotential (:2319-2343), over the dense grid of include/mtg.h.

Two models share one loop, written over an arithmetic (Python floats = IEEE FP64 without FMA, or
mpmath at 50 digits):

* fp64_model: the literal restatement.  Coefficients from the library's
  mtg_host_coefficients_from_vertices_batch.  It also returns the per-sample gate decisions, S_J (the
  sum of |cost terms|), S_g (per gradient entry, the sum over samples of |the sample's contribution|)
  and the smallest margin of every comparison the loop makes on a rounded quantity: t < T_i,
  time_sum < 0, dist_sum < map_resolution, the bounds test, the distance of every lookup position to a
  cell boundary (in cell units), d <= 0 of the flag, |vel| > 1e-6.
* truth_model: the same terms in 50 digits from the vertex values (coefficients by an exact-to-50-
  digits solve with A(T)), with the FP64 model's sample clock and gate decisions taken as fixed.

The triLerp pairing is kept as the reference wrote it (its y step joins x00 with x01 and x10 with
x11), so on the planar field distance = z the continuous lookup returns z_c + (y - y_c) of the cell
(c = centre), not z: it is exact only for fields linear in x.
"""
import functools
import math

import numpy as np

from mav_trajectory_generation_cmake_amd import _native as nat

try:
    import mpmath
except ImportError:  # the truth tests need it; the others do not
    mpmath = None


class Grid:
    def __init__(self, field, origin, resolution, oob):
        self.field = np.ascontiguousarray(field, dtype=np.float32)
        self.origin = tuple(float(o) for o in origin)
        self.resolution = float(resolution)
        self.oob = float(oob)


class Params:
    def __init__(self, dt, map_resolution, epsilon, robot_radius, multiplier, lo, hi, continuous):
        self.dt, self.map_resolution, self.epsilon = float(dt), float(map_resolution), float(epsilon)
        self.robot_radius, self.multiplier = float(robot_radius), float(multiplier)
        self.lo, self.hi = tuple(float(v) for v in lo), tuple(float(v) for v in hi)
        self.continuous = bool(continuous)


class _F64:
    F = float
    floor = staticmethod(math.floor)
    sqrt = staticmethod(math.sqrt)
    nan = float("nan")


class _MP:
    @staticmethod
    def F(v):
        return mpmath.mpf(v)

    @staticmethod
    def floor(v):
        return int(mpmath.floor(v))

    @staticmethod
    def sqrt(v):
        return mpmath.sqrt(v)

    nan = None  # set on first use


class _Margins:
    def __init__(self):
        self.by_kind = {}
        self.band = math.inf  # min over every lookup of min(d, epsilon - d): > 0 = all in the quadratic band

    def add(self, kind, value):
        value = abs(float(value))
        if value < self.by_kind.get(kind, math.inf):
            self.by_kind[kind] = value

    def smallest(self):
        return min(self.by_kind.values()) if self.by_kind else math.inf


def _distance(ar, grid, p, continuous, rec, kind="cell"):
    F = ar.F
    res = F(grid.resolution)
    n = grid.field.shape
    c = []
    for k in range(3):
        u = (p[k] - F(grid.origin[k])) / res
        f = ar.floor(u)
        if rec is not None:
            frac = float(u - f)
            rec.add(kind, min(frac, 1.0 - frac))
        c.append(int(f))
    if not all(0 <= c[k] < n[k] for k in range(3)):
        return F(grid.oob)
    at = lambda ix, iy, iz: F(float(grid.field[ix, iy, iz]))
    corners = all(1 <= c[k] <= n[k] - 2 for k in range(3))
    if not continuous or not corners:
        return at(c[0], c[1], c[2])
    w0, w1 = [], []
    for k in range(3):
        x1 = F(grid.origin[k]) + (F(c[k] - 1) + F(0.5)) * res
        x2 = F(grid.origin[k]) + (F(c[k] + 1) + F(0.5)) * res
        w0.append((x2 - p[k]) / (x2 - x1))
        w1.append((p[k] - x1) / (x2 - x1))
    q = lambda a, b, d: at(c[0] + a, c[1] + b, c[2] + d)
    # triLerp (:2451-2464) as written
    x00 = w0[0] * q(-1, -1, -1) + w1[0] * q(+1, -1, -1)
    x10 = w0[0] * q(-1, +1, -1) + w1[0] * q(+1, +1, -1)
    x01 = w0[0] * q(-1, -1, +1) + w1[0] * q(+1, -1, +1)
    x11 = w0[0] * q(-1, +1, +1) + w1[0] * q(+1, +1, +1)
    r0 = w0[1] * x00 + w1[1] * x01
    r1 = w0[1] * x10 + w1[1] * x11
    return w0[2] * r0 + w1[2] * r1


def _potential(ar, prm, distance):
    F = ar.F
    d = distance - F(prm.robot_radius)
    if d <= 0:
        return F(prm.multiplier) * (-d) + F(0.5) * F(prm.epsilon), True, d
    if d <= F(prm.epsilon):
        e = d - F(prm.epsilon)
        return F(0.5) * F(1.0) / F(prm.epsilon) * e * e, False, d
    return F(0.0), False, d


def _potential_at(ar, grid, prm, p, want_grad, rec):
    F = ar.F
    inc = F(prm.map_resolution)
    valid = True
    for k in range(3):
        lo, hi = F(prm.lo[k]) + inc, F(prm.hi[k]) - inc
        if rec is not None:
            rec.add("bounds", p[k] - lo)
            rec.add("bounds", hi - p[k])
        if p[k] < lo or p[k] > hi:
            valid = False
    cont = valid and prm.continuous
    c, coll, d = _potential(ar, prm, _distance(ar, grid, p, cont, rec, "cell_unshifted"))
    if rec is not None:
        rec.add("flag", d)
        rec.band = min(rec.band, float(d), prm.epsilon - float(d))
    g = [F(0.0)] * 3
    if want_grad:
        for k in range(3):
            pl, pr = list(p), list(p)
            pl[k] = p[k] - inc
            pr[k] = p[k] + inc
            left, _, dl = _potential(ar, prm, _distance(ar, grid, pl, cont, rec))
            right, _, dr = _potential(ar, prm, _distance(ar, grid, pr, cont, rec))
            if rec is not None:
                rec.band = min(rec.band, float(dl), prm.epsilon - float(dl), float(dr), prm.epsilon - float(dr))
            g[k] = (right - left) / (F(2.0) * inc) if prm.map_resolution != 0.0 else ar.nan  # 0 / 0
    return c, g, coll


def _loop(ar, N, coeffs, times, grid, prm, want_grad, forced=None, rec=None):
    """The reference loop.  forced: the decisions (0 first entry, 1 gated, 2 evaluated) to follow
    instead of the comparisons; rec: a _Margins to fill.  Returns a dict; `vectors` is, per evaluated
    sample, (segment, [3][N] contribution to the segment's coefficient-space vectors)."""
    F = ar.F
    K = len(times)
    dt, gate = F(prm.dt), F(prm.map_resolution)
    J, S_J = F(0.0), F(0.0)
    flag, n_eval = False, 0
    decisions, vectors = [], []
    prev = [F(0.0)] * 3
    time_sum, dist_sum = F(-1.0), F(0.0)
    idx = 0
    for i in range(K):
        T = times[i]
        t = 0.0  # the clock is FP64 in both models
        entering = True  # time_sum is a rounded sum only at a segment's first sample
        while True:
            if rec is not None:
                rec.add("clock", t - T)
            if not t < T:
                break
            tt = F(t)
            pos, vel = [], []
            for k in range(3):
                c = coeffs[i][k]
                p, v = c[N - 1], F(N - 1) * c[N - 1]
                for n in range(N - 2, -1, -1):
                    p = p * tt + c[n]
                for n in range(N - 2, 0, -1):
                    v = v * tt + F(n) * c[n]
                pos.append(p)
                vel.append(v)
            if rec is not None and entering:
                rec.add("first", time_sum)
            entering = False
            first = forced[idx] == 0 if forced is not None else time_sum < 0
            if first:
                time_sum = F(0.0)
                prev = pos
                decisions.append(0)
                idx += 1
                t += prm.dt
                continue
            time_sum = time_sum + dt
            dx, dy, dz = pos[0] - prev[0], pos[1] - prev[1], pos[2] - prev[2]
            dist_sum = dist_sum + ar.sqrt(dx * dx + dy * dy + dz * dz)
            prev = pos
            if rec is not None:
                rec.add("gate", dist_sum - gate)
            gated = forced[idx] == 1 if forced is not None else dist_sum < gate
            if gated:
                decisions.append(1)
                idx += 1
                t += prm.dt
                continue
            decisions.append(2)
            idx += 1
            c, gc, coll = _potential_at(ar, grid, prm, pos, want_grad, rec)
            flag = flag or coll
            n_eval += 1
            vn = ar.sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2])
            term = c * vn * time_sum
            J = J + term
            S_J = S_J + abs(term)
            if rec is not None:
                rec.add("velocity", vn - F(1e-6))
            if want_grad and vn > F(1e-6):
                vec = []
                for k in range(3):
                    a = vn * time_sum * gc[k]
                    b = time_sum * c * vel[k] / vn
                    tp, tm, row = F(1.0), F(0.0), []
                    for n in range(N):
                        row.append(a * tp + b * (F(n) * tm))
                        tm = tp
                        tp = tp * tt
                    vec.append(row)
                vectors.append((i, vec))
            dist_sum = F(0.0)
            time_sum = F(0.0)
            t += prm.dt
        time_sum = time_sum + (-dt + (F(T) - F(t)))
    return {"J": J, "S_J": S_J, "flag": flag, "n_eval": n_eval, "decisions": decisions, "vectors": vectors}


def host_coefficients(N, x, times):
    """[K][3][N] from the library's mtg_host_coefficients_from_vertices_batch."""
    lib = nat.load()
    x = np.ascontiguousarray(x, dtype=np.float64)[None]
    times = np.ascontiguousarray(times, dtype=np.float64)[None]
    K = times.shape[1]
    out = np.empty((1, K, 3, N))
    nat.check(lib.mtg_host_coefficients_from_vertices_batch(N, 3, K, 1, x.ctypes.data, times.ctypes.data,
                                                            out.ctypes.data, 1))
    return out[0]


def _a_inverse(N, T):
    out = np.empty((N, N))
    nat.check(nat.load().mtg_host_segment_matrices(N, 0, float(T), None, out.ctypes.data, None, None))
    return out


def _pack(N, K, mask, seg, zero, add=lambda a, b: a + b):
    """seg [K][3][N] = A^-T of the segment vectors -> [3][list of free entries], free order."""
    h = N // 2
    out = []
    for k in range(3):
        g = []
        for v in range(K + 1):
            for q in range(h):
                if (int(mask[v]) >> q) & 1:
                    continue
                bot = seg[v - 1][k][h + q] if v > 0 else zero
                top = seg[v][k][q] if v < K else zero
                g.append(add(bot, top))
        out.append(g)
    return out


def fp64_model(N, x, times, mask, grid, prm, want_grad=True):
    """x [V][h][3] all vertex derivatives, times [K], mask [V].  Returns dict(cost, grad [3][V*h], flag,
    n_eval, decisions, S_J, S_g [3][V*h], margin, margins)."""
    x = np.asarray(x, dtype=np.float64)
    times = [float(t) for t in times]
    K, h = len(times), N // 2
    co = host_coefficients(N, x, times)
    coeffs = [[[float(v) for v in co[i, k]] for k in range(3)] for i in range(K)]
    rec = _Margins()
    r = _loop(_F64, N, coeffs, times, grid, prm, want_grad, rec=rec)
    out = {"cost": r["J"], "flag": r["flag"], "n_eval": r["n_eval"], "decisions": r["decisions"], "S_J": r["S_J"],
           "margin": rec.smallest(), "margins": rec.by_kind, "band": rec.band}
    if want_grad:
        ainv_t = [_a_inverse(N, T).T for T in times]
        seg = np.zeros((K, 3, N))
        seg_abs = np.zeros((K, 3, N))
        acc = np.zeros((K, 3, N))
        for i, vec in r["vectors"]:  # the loop's own order of summation
            acc[i] += np.array(vec)
        for i in range(K):
            for k in range(3):
                seg[i, k] = ainv_t[i] @ acc[i, k]
        for i, vec in r["vectors"]:
            for k in range(3):
                seg_abs[i, k] += np.abs(ainv_t[i] @ np.array(vec[k]))
        V = K + 1
        grad, S_g = np.zeros((3, V * h)), np.zeros((3, V * h))
        for k, g in enumerate(_pack(N, K, mask, seg, 0.0)):
            grad[k, :len(g)] = g
        for k, g in enumerate(_pack(N, K, mask, seg_abs, 0.0)):
            S_g[k, :len(g)] = g
        out["grad"], out["S_g"] = grad, S_g
    return out


def _mp_mapping(N, T):
    """A(T) (setupMappingMatrix, lin_impl:102-111) in mpmath."""
    h = N // 2
    A = mpmath.zeros(N, N)
    for k in range(h):
        for j in range(k, N):
            f = mpmath.mpf(1)
            for q in range(k):
                f *= j - q
            A[h + k, j] = f * T ** (j - k)
            if j == k:
                A[k, j] = f
    return A


def truth_model(N, x, times, mask, grid, prm, decisions, want_grad=True):
    """The same terms at 50 digits, following `decisions`.  Returns dict(cost, grad [3][V*h]) as
    mpmath numbers / lists."""
    with mpmath.workdps(50):
        _MP.nan = mpmath.nan
        x = np.asarray(x, dtype=np.float64)
        K, h = len(times), N // 2
        A = [_mp_mapping(N, mpmath.mpf(float(T))) for T in times]
        coeffs = []
        for i in range(K):
            rows = []
            for k in range(3):
                rhs = mpmath.matrix([mpmath.mpf(float(x[i, q, k])) for q in range(h)] +
                                    [mpmath.mpf(float(x[i + 1, q, k])) for q in range(h)])
                sol = mpmath.lu_solve(A[i], rhs)
                rows.append([sol[j] for j in range(N)])
            coeffs.append(rows)
        r = _loop(_MP, N, coeffs, [float(t) for t in times], grid, prm, want_grad, forced=decisions)
        assert r["decisions"] == list(decisions)
        out = {"cost": r["J"], "flag": r["flag"]}
        if want_grad:
            zero = mpmath.mpf(0)
            acc = [[[zero] * N for _ in range(3)] for _ in range(K)]
            for i, vec in r["vectors"]:
                for k in range(3):
                    acc[i][k] = [a + b for a, b in zip(acc[i][k], vec[k])]
            seg = []
            for i in range(K):
                rows = []
                for k in range(3):
                    if any(mpmath.isnan(v) for v in acc[i][k]):
                        rows.append([mpmath.nan] * N)
                        continue
                    y = mpmath.lu_solve(A[i].T, mpmath.matrix(acc[i][k]))
                    rows.append([y[j] for j in range(N)])
                seg.append(rows)
            V = K + 1
            grad = [[zero] * (V * h) for _ in range(3)]
            for k, g in enumerate(_pack(N, K, mask, seg, zero)):
                grad[k][:len(g)] = g
            out["grad"] = grad
        return out


def check_against(name, got_cost, got_grad, model, truth=None, model_tol=1e-6, truth_tol=1e-9):
    """The acceptance measures: against the FP64 model error <= 1e-6 S; against the truth error <=
    max(4 x the model's own error, 1e-9 S); S = S_J for the cost, the per-axis maximum of S_g for the
    gradient.  NaN entries (map_resolution == 0) must coincide.  Prints each figure, then asserts.
    Returns the worst ratios (error / bound)."""
    worst = {}
    S = model["S_J"]
    e = abs(got_cost - model["cost"])
    print("%s cost: |got - model| = %.3e, bound %.3e" % (name, e, model_tol * S))
    fails = []
    if not e <= model_tol * S:
        fails.append("cost vs model")
    worst["cost_model"] = e / (model_tol * S) if S > 0 else 0.0
    if truth is not None:
        with mpmath.workdps(50):
            et = float(abs(mpmath.mpf(float(got_cost)) - truth["cost"]))
            em = float(abs(mpmath.mpf(float(model["cost"])) - truth["cost"]))
        bound = max(4.0 * em, truth_tol * S)
        print("%s cost: |got - truth| = %.3e, model's own %.3e, bound %.3e" % (name, et, em, bound))
        if not et <= bound:
            fails.append("cost vs truth")
        worst["cost_truth"] = et / bound if bound > 0 else 0.0
    if got_grad is not None:
        got_grad = np.asarray(got_grad)
        mg = model["grad"]
        nan_m, nan_g = np.isnan(mg), np.isnan(got_grad)
        if not (nan_m == nan_g).all():
            fails.append("NaN pattern of the gradient")
        for k in range(3):
            Sk = float(np.max(model["S_g"][k][~nan_m[k]])) if (~nan_m[k]).any() else 0.0
            ok = ~nan_m[k] & ~nan_g[k]
            e = float(np.max(np.abs(got_grad[k][ok] - mg[k][ok]))) if ok.any() else 0.0
            print("%s grad axis %d: max |got - model| = %.3e, bound %.3e" % (name, k, e, model_tol * Sk))
            if not e <= model_tol * Sk:
                fails.append("grad axis %d vs model" % k)
            worst["grad_model"] = max(worst.get("grad_model", 0.0), e / (model_tol * Sk) if Sk > 0 else 0.0)
            if truth is not None:
                with mpmath.workdps(50):
                    for j in np.flatnonzero(ok):
                        tv = truth["grad"][k][j]
                        if mpmath.isnan(tv):
                            fails.append("truth NaN where the model is finite")
                            continue
                        et = float(abs(mpmath.mpf(float(got_grad[k][j])) - tv))
                        em = float(abs(mpmath.mpf(float(mg[k][j])) - tv))
                        bound = max(4.0 * em, truth_tol * Sk)
                        if not et <= bound:
                            print("%s grad[%d][%d]: |got - truth| = %.3e, model's own %.3e, bound %.3e"
                                  % (name, k, j, et, em, bound))
                            fails.append("grad[%d][%d] vs truth" % (k, j))
                        worst["grad_truth"] = max(worst.get("grad_truth", 0.0), et / bound if bound > 0 else 0.0)
    print("%s worst ratios: %s" % (name, {k: "%.3g" % v for k, v in worst.items()}))
    assert not fails, (name, fails)
    return worst


# ----------------------------------------------------------------------------- maps and cases
def sphere_map(n=64, origin=-8.0, resolution=0.25, seed=7, spheres=12):
    """Union of spheres min_i(|p - c_i| - r_i) at the cell centres, float32."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(origin + 2.0, origin + n * resolution - 2.0, size=(spheres, 3))
    radii = rng.uniform(0.5, 1.5, size=spheres)
    ax = origin + (np.arange(n) + 0.5) * resolution
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    d = np.full((n, n, n), np.inf)
    for c, r in zip(centres, radii):
        d = np.minimum(d, np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r)
    return Grid(d.astype(np.float32), (origin,) * 3, resolution, 0.75)


def planar_map(n=64, origin=-8.0, resolution=0.25):
    """distance = z of the cell centre: every value exact in float32."""
    z = (origin + (np.arange(n) + 0.5) * resolution).astype(np.float32)
    return Grid(np.broadcast_to(z, (n, n, n)).copy(), (origin,) * 3, resolution, 100.0)


def random_trajectory(N, K, seed, times, extent=5.0, mask=None):
    """Vertex values [V][h][3] (all derivatives given) of a smooth random trajectory inside
    [-extent, extent]^3, and a mask: the ends fix everything, interior vertices their position."""
    rng = np.random.default_rng(seed)
    h, V = N // 2, K + 1
    x = np.zeros((V, h, 3))
    x[:, 0] = rng.uniform(-extent, extent, size=(V, 3))
    step = np.diff(x[:, 0], axis=0)
    for v in range(V):
        T = times[min(v, K - 1)]
        x[v, 1] = (step[min(v, K - 1)] / T) * rng.uniform(0.5, 1.0)
        for q in range(2, h):
            x[v, q] = rng.normal(size=3) * 0.3 / T ** (q - 1)
    if mask is None:
        mask = np.full(V, 1, dtype=np.uint8)
        mask[0] = mask[-1] = (1 << h) - 1
    return x, np.asarray(mask, dtype=np.uint8)


def to_native(grid, prm):
    """(mtg.SdfGrid, mtg.CollisionParams) of a model Grid / Params."""
    import mav_trajectory_generation_cmake_amd as mtg
    return (mtg.SdfGrid(grid.field, grid.origin, grid.resolution, grid.oob),
            mtg.CollisionParams(prm.dt, prm.map_resolution, prm.epsilon, prm.robot_radius, prm.multiplier, prm.lo, prm.hi,
                                prm.continuous))


@functools.lru_cache(maxsize=None)
def maps():
    return {"sphere": sphere_map(), "plane": planar_map()}


def _case(name, N, K, times, seed, grid, dt, map_resolution, continuous, extent=5.0, bound=7.0, interior_mask=1,
          epsilon=1.0, radius=0.3):
    return dict(name=name, N=N, K=K, times=tuple(times), seed=seed, grid=grid, dt=dt, map_resolution=map_resolution,
                continuous=continuous, extent=extent, bound=bound, interior_mask=interior_mask, epsilon=epsilon,
                radius=radius)


# The cases of the host / device comparison (test 3 / 6 of the collision tests): the smallest shapes
# at which each path of the loop is taken.  Seeds were chosen on the CPU so that the FP64 model's
# smallest margin is >= 1e-9 (asserted by the tests).
CASES = [
    _case("k1", 10, 1, (2.33,), 1, "sphere", 0.1, 0.2, True),
    _case("k2-interior", 10, 2, (1.74, 2.17), 2, "sphere", 0.1, 0.2, True),
    _case("short-segment", 10, 3, (1.33, 0.07, 1.46), 3, "sphere", 0.1, 0.1, False),
    _case("dt-0.125", 10, 2, (1.3, 2.2), 4, "sphere", 0.125, 0.2, True),
    _case("mostly-gated", 10, 2, (2.13, 1.94), 5, "sphere", 0.1, 1.5, True),
    _case("nothing-gated", 10, 2, (1.13, 1.36), 6, "sphere", 0.1, 0.0, True),
    _case("leaves-grid", 10, 2, (2.33, 2.64), 7, "sphere", 0.1, 0.2, True, extent=11.0, bound=7.0),
    _case("nearest", 10, 2, (1.93, 1.66), 8, "sphere", 0.1, 0.2, False),
    _case("n6-k3", 6, 3, (1.23, 1.74, 1.46), 9, "sphere", 0.1, 0.2, True),
    _case("n12-k3", 12, 3, (1.63, 1.24, 1.96), 10, "sphere", 0.1, 0.2, True),
    _case("fixed-interior-velocity", 8, 3, (1.53, 1.84, 1.36), 11, "sphere", 0.1, 0.2, True, interior_mask=3),
    _case("plane-continuous", 10, 2, (1.44, 1.83), 12, "plane", 0.1, 0.2, True, extent=3.0),
]


@functools.lru_cache(maxsize=None)
def build_case(name, n_traj=4):
    """The inputs of a case: n_traj trajectories (seeds seed*100 + j), its grid and parameters, and the
    FP64 model of every trajectory (computed once per session, shared by the host and device tests)."""
    case = next(c for c in CASES if c["name"] == name)
    N, K = case["N"], case["K"]
    h, V = N // 2, K + 1
    grid = maps()[case["grid"]]
    b = case["bound"]
    prm = Params(case["dt"], case["map_resolution"], case["epsilon"], case["radius"], 2.0, (-b,) * 3, (b,) * 3,
                 case["continuous"])
    mask = np.full(V, case["interior_mask"], dtype=np.uint8)
    mask[0] = mask[-1] = (1 << h) - 1
    xs, models = [], []
    for j in range(n_traj):
        x, _ = random_trajectory(N, K, case["seed"] * 100 + j, case["times"], extent=case["extent"], mask=mask)
        xs.append(x)
        models.append(fp64_model(N, x, case["times"], mask, grid, prm))
    return dict(case=case, N=N, K=K, x=np.array(xs), times=np.tile(np.array(case["times"]), (n_traj, 1)),
                mask=np.tile(mask, (n_traj, 1)), grid=grid, prm=prm, models=models)


@functools.lru_cache(maxsize=None)
def case_truth(name, j):
    c = build_case(name)
    return truth_model(c["N"], c["x"][j], c["case"]["times"], c["mask"][j], c["grid"], c["prm"],
                       tuple(c["models"][j]["decisions"]))
