"""The host-pointer staging and the argument checks of the C ABI (csrc/mtg_capi.hip), pinned through
ctypes so that optional pointers are really NULL: which optional outputs are present must not change
any other output's bits, every output is written with exactly its byte count, device-pointer calls
return the host-pointer call's bits, a staging buffer that grew and is reused returns the same bits,
and every argument check returns its code and its mtg_last_error text.

Shapes are the smallest that reach every staged array: B = 3, N = 6 and 10, K = 2, D = 3, an 8x8x8
grid; one B = 67 objective call makes the staging buffer grow.

Not in the validation table: the HIP runtime failures (they cannot be provoked without a fault)."""
import ctypes
import functools

import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _collision_model as M
import _objective_cases as OC

pytestmark = pytest.mark.gpu

B, K, D = 3, 2, 3
TIMES = (1.74, 2.17)
GUARD = 64
SENTINEL = np.uint64(0x7FF8DEADBEEFCAFE)  # a NaN with a distinctive payload
DEV, ASYNC = nat.MTG_FLAG_DEVICE_PTRS, nat.MTG_FLAG_ASYNC
PARTS = mtg.solver.OBJECTIVE_PARTS


class Guarded:
    """An output array inside a larger buffer filled with the sentinel, GUARD bytes on both sides."""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.raw = np.full((2 * GUARD + self.n + 7) // 8, SENTINEL, np.uint64).view(np.uint8)
        self.arr = self.raw[GUARD:GUARD + self.n].view(dtype).reshape(shape)
        self.item = np.dtype(dtype).itemsize

    def check(self, label, written=True):
        fresh = np.full(self.raw.size // 8, SENTINEL, np.uint64).view(np.uint8)
        assert self.raw[:GUARD].tobytes() == fresh[:GUARD].tobytes(), (label, "guard below")
        assert self.raw[GUARD + self.n:].tobytes() == fresh[GUARD + self.n:].tobytes(), (label, "guard above")
        if written:  # no element still holds the bytes the buffer was filled with
            got = self.raw[GUARD:GUARD + self.n].reshape(-1, self.item)
            was = fresh[GUARD:GUARD + self.n].reshape(-1, self.item)
            assert not (got == was).all(axis=1).any(), (label, "an element was not written")


class Entry:
    """One entry point: its host inputs, its outputs name -> (shape, dtype), which are optional, and
    call(lib, handle, a, flags) with a = name -> address or None."""

    def __init__(self, name, inputs, outs, optional, call, inout=None, groups=None):
        self.name, self.inputs, self.outs, self.optional, self.call = name, inputs, outs, tuple(optional), call
        self.inout = inout or {}    # name -> initial contents (read and written)
        self.groups = groups or {}  # an optional that stands for several arrays: name -> f(present) -> names
        grouped = {k for f in self.groups.values() for k in f(self.optional)}
        self.required = [k for k in outs if k not in self.optional and k not in grouped]

    def wanted(self, present):
        names = list(self.required)
        for k in present:
            names += self.groups[k](present) if k in self.groups else [k]
        return names


def _rc(ctx, rc):
    assert rc == nat.MTG_OK, (rc, nat.load().mtg_last_error(ctx).decode())


def host_call(ctx, e, present):
    """A host-pointer call with the optional outputs `present`; every output sits between guards."""
    bufs = {k: Guarded(*e.outs[k]) for k in e.wanted(present)}
    for k, v in e.inout.items():
        if k in bufs:
            bufs[k].arr[...] = v
    a = {k: v.ctypes.data for k, v in e.inputs.items()}
    a.update({k: bufs[k].arr.ctypes.data if k in bufs else None for k in e.outs})
    _rc(ctx, e.call(nat.load(), ctx, a, 0))
    for k, b in bufs.items():
        b.check((e.name, tuple(present), k), written=k not in e.inout)
    return {k: b.arr.tobytes() for k, b in bufs.items()}


def device_call(ctx, e, present, flags):
    """The same call on torch device memory; with MTG_FLAG_ASYNC the stream is synchronised after it."""
    import torch
    dv = torch.device("cuda", 0)
    ins = {k: torch.from_numpy(v).to(dv) for k, v in e.inputs.items()}
    outs = {}
    for k in e.wanted(present):
        shape, dtype = e.outs[k]
        host = np.zeros(shape, dtype)
        if k in e.inout:
            host[...] = e.inout[k]
        outs[k] = torch.from_numpy(host.view(np.uint8).reshape(-1)).to(dv)
    a = {k: v.data_ptr() for k, v in ins.items()}
    a.update({k: outs[k].data_ptr() if k in outs else None for k in e.outs})
    _rc(ctx, e.call(nat.load(), ctx, a, flags))
    if flags & ASYNC:
        _rc(ctx, nat.load().mtg_synchronize(ctx))
    return {k: t.cpu().numpy().tobytes() for k, t in outs.items()}


@functools.lru_cache(maxsize=None)
def case(N):
    """The objective-test inputs (tests/_objective_cases.py) of B trajectories of order N over a small grid."""
    xs = np.array([M.random_trajectory(N, K, 9100 + 10 * N + j, TIMES)[0] for j in range(B)])
    masks = np.tile(M.random_trajectory(N, K, 0, TIMES)[1], (B, 1))
    times = np.tile(np.array(TIMES), (B, 1)) * (1.0 + 0.01 * np.arange(B))[:, None]
    c = OC._finish("staging%d" % N, N, xs, masks, times, M.Params(0.1, 0.2, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True))
    c["grid"] = M.sphere_map(n=8, origin=-8.0, resolution=2.0, spheres=4)
    h = N // 2
    coeffs = np.empty((B, K, D, N))
    nat.check(nat.load().mtg_host_coefficients_from_vertices_batch(N, D, K, B, xs.ctypes.data, times.ctypes.data,
                                                                   coeffs.ctypes.data, 1))
    c.update(coeffs=coeffs, scales=np.array([[1.0, 1.0], [0.9, 1.2]]), h=h)
    return c


def _grid(c, address):
    g = c["grid"]
    nx, ny, nz = g.field.shape
    return nat.SdfGrid(address, nx, ny, nz, (ctypes.c_double * 3)(*g.origin), g.resolution, g.oob)


def _byref(s):
    return ctypes.byref(s) if s is not None else None


def objective_entry(c, objective=2):
    N, Bc, Kc, h, stride = c["N"], c["B"], c["K"], c["N"] // 2, c["stride"]
    V = Kc + 1
    p = OC.params(c, objective).native()
    cp, sp = c["p"].native(), c["soft"].native().native()
    inputs = dict(values=c["values"], mask=c["mask"], x=np.ascontiguousarray(OC.x_of(c, objective)), grid=c["grid"].field)
    if objective != 2:
        inputs["times"] = c["times"]
    shapes = {"J_d": (Bc,), "J_c": (Bc,), "J_sc": (Bc,), "J_t": (Bc,), "dJd_dt": (Bc, Kc), "dJc_dt": (Bc, Kc),
              "grad_d": (Bc, D, V * h), "grad_c": (Bc, D, V * h), "grad_sc": (Bc, D, V * h)}
    outs = dict(cost=((Bc,), np.float64), grad=((Bc, stride), np.float64), weighted=((Bc, 4), np.float64),
                collision=((Bc,), np.uint8), state=((Bc,), mtg.OBJECTIVE_STATE_DTYPE), status=((Bc,), np.int32))
    outs.update({k: (s, np.float64) for k, s in shapes.items()})
    state = OC.zero_state(Bc)
    state["n_iterations"] = 3 + np.arange(Bc)

    def parts(present):  # the gradient parts exist only with grad_out
        return list(PARTS) if "grad" in present else ["J_d", "J_c", "J_sc", "J_t"]

    def call(lib, ctx, a, flags):
        g = _grid(c, a["grid"])
        pp = nat.ObjectiveParts(*[a[k] for k in PARTS])
        return lib.mtg_objective_batch(ctx, N, D, Kc, Bc, a["values"], a["mask"], a.get("times"), a["x"], stride,
                                       ctypes.byref(p), ctypes.byref(g), ctypes.byref(cp), ctypes.byref(sp), a["cost"],
                                       a["grad"], a["weighted"], a["collision"], a["state"],
                                       ctypes.byref(pp) if any(a[k] for k in PARTS) else None, a["status"], flags)

    return Entry("objective", inputs, outs, ("grad", "weighted", "collision", "state", "status", "parts"), call,
                 inout={"state": state}, groups={"parts": parts})


@functools.lru_cache(maxsize=None)
def entries(N):
    c = case(N)
    h, V, r, C = N // 2, K + 1, c["r"], 2
    x, mask, times, coeffs, scales = c["full"], c["mask"], c["times"], c["coeffs"], c["scales"]
    cp, sp = c["p"].native(), c["soft"].native().native()
    f8, i4, u1, ext = np.float64, np.int32, np.uint8, mtg.solver.EXTREMUM_DTYPE
    out = []

    def call(lib, ctx, a, flags):
        return lib.mtg_cost_at_times_batch(ctx, N, D, K, r, B, a["x"], a["mask"], a["times"], C, a["scales"], a["cost"],
                                           a["grad"], flags)
    out.append(Entry("cost_at_times", dict(x=x, mask=mask, times=times, scales=scales),
                     dict(cost=((B, C), f8), grad=((B, C, D, V * h), f8)), ("grad",), call))

    def call(lib, ctx, a, flags):
        g = _grid(c, a["grid"])
        return lib.mtg_collision_cost_batch(ctx, N, D, K, B, a["x"], a["mask"], a["times"], ctypes.byref(g), ctypes.byref(cp),
                                            a["cost"], a["grad"], a["collision"], a["n_evaluated"], a["status"], flags)
    out.append(Entry("collision", dict(x=x, mask=mask, times=times, grid=c["grid"].field),
                     dict(cost=((B,), f8), grad=((B, D, V * h), f8), collision=((B,), u1), n_evaluated=((B,), i4),
                          status=((B,), i4)), ("grad", "collision", "n_evaluated", "status"), call))

    def call(lib, ctx, a, flags):
        g = _grid(c, a["grid"])
        return lib.mtg_collision_time_gradient_batch(ctx, N, D, K, B, a["x"], a["times"], ctypes.byref(g), ctypes.byref(cp),
                                                     0.1, a["grad_t"], a["side_cost"], a["side_evaluated"],
                                                     a["segments_walked"], a["status"], flags)
    out.append(Entry("collision_time", dict(x=x, times=times, grid=c["grid"].field),
                     dict(grad_t=((B, K), f8), side_cost=((B, K, 2), f8), side_evaluated=((B, K, 2), i4),
                          segments_walked=((B,), i4), status=((B,), i4)),
                     ("side_cost", "side_evaluated", "segments_walked", "status"), call))

    def call(lib, ctx, a, flags):
        return lib.mtg_soft_constraint_cost_batch(ctx, N, D, K, B, a["x"], a["mask"], a["times"], ctypes.byref(sp), a["cost"],
                                                  a["grad"], a["maxima"], a["status"], flags)
    out.append(Entry("soft_constraint", dict(x=x, mask=mask, times=times),
                     dict(cost=((B,), f8), grad=((B, D, V * h), f8), maxima=((B, sp.n_constraints), ext), status=((B,), i4)),
                     ("grad", "maxima", "status"), call))

    def call(lib, ctx, a, flags):
        return lib.mtg_time_jacobian_batch(ctx, N, D, K, r, B, a["x"], a["times"], C, a["scales"], 0.1, a["cost"], a["jac"],
                                           flags)
    out.append(Entry("time_jacobian", dict(x=x, times=times, scales=scales),
                     dict(cost=((B, C), f8), jac=((B, C, K), f8)), ("jac",), call))

    def call(lib, ctx, a, flags):
        return lib.mtg_coefficients_from_vertices_batch(ctx, N, D, K, B, a["x"], a["times"], a["coeffs"], flags)
    out.append(Entry("coefficients_from_vertices", dict(x=x, times=times), dict(coeffs=((B, K, D, N), f8)), (), call))

    def call(lib, ctx, a, flags):
        return lib.mtg_vertex_derivatives_batch(ctx, N, D, K, B, a["coeffs"], a["times"], a["x"], flags)
    out.append(Entry("vertex_derivatives", dict(coeffs=coeffs, times=times), dict(x=((B, V, h, D), f8)), (), call))

    def call(lib, ctx, a, flags):
        return lib.mtg_min_max_magnitude_batch(ctx, N, D, K, B, a["coeffs"], a["times"], 1, 0, a["minimum"], a["maximum"],
                                               flags)
    out.append(Entry("min_max", dict(coeffs=coeffs, times=times), dict(minimum=((B,), ext), maximum=((B,), ext)),
                     ("minimum", "maximum"), call))
    out.append(objective_entry(c))
    return {e.name: e for e in out}


NAMES = ("cost_at_times", "collision", "collision_time", "soft_constraint", "time_jacobian",
         "coefficients_from_vertices", "vertex_derivatives", "min_max", "objective")


@pytest.mark.parametrize("N", (6, 10))
@pytest.mark.parametrize("name", NAMES)
def test_optional_outputs_and_byte_counts(gpu_ctx, name, N):
    """Items 1 and 2: every optional output present, none, and each alone; the guards of every output
    buffer are intact and every element of it was written (host_call checks both)."""
    gpu_ctx.reset_stream()
    e = entries(N)[name]
    full = host_call(gpu_ctx.handle, e, e.optional)
    assert set(full) == set(e.outs)
    for present in [()] + [(k,) for k in e.optional]:
        got = host_call(gpu_ctx.handle, e, present)
        assert set(got) >= set(e.required)
        for k, v in got.items():
            assert v == full[k], (name, present, k)


@pytest.mark.parametrize("N", (6, 10))
@pytest.mark.parametrize("name", ("cost_at_times", "time_jacobian", "coefficients_from_vertices", "vertex_derivatives",
                                  "min_max"))
def test_device_pointers_same_bits(gpu_ctx, name, N):
    """Item 3: device pointers, synchronous and MTG_FLAG_ASYNC + a stream synchronise, against the
    host-pointer call; without the optional outputs too (cost_at_times then passes a fixed_mask that
    nothing reads)."""
    gpu_ctx.reset_stream()
    e = entries(N)[name]
    for present in (e.optional, ()):
        want = host_call(gpu_ctx.handle, e, present)
        for flags in (DEV, DEV | ASYNC):
            got = device_call(gpu_ctx.handle, e, present, flags)
            for k in want:
                assert got[k] == want[k], (name, present, flags, k)


def test_staging_reuse_same_bits():
    """Item 4: on one context a B = 67 objective call grows the staging buffer, then every entry runs at
    B = 3 in the larger buffer, then the objective again; four times, always the first round's bits."""
    big = objective_entry(OC.shape("batch67"))
    small = [e for N in (6, 10) for e in entries(N).values()]
    with mtg.Context(0) as ctx:
        first = None
        for _ in range(4):
            got = [host_call(ctx.handle, big, big.optional)]
            got += [host_call(ctx.handle, e, e.optional) for e in small]
            got.append(host_call(ctx.handle, big, big.optional))
            if first is None:
                first = got
            for i, (a, b) in enumerate(zip(got, first)):
                assert a == b, i
        # the state is an input too: both objective calls of a round started from the same one
        assert first[0] == first[-1]


# ----------------------------------------------------------------------------- item 5: the validation table
INV, UNS, BAD, SIZE, BIG = (nat.MTG_ERR_INVALID_ARGUMENT, nat.MTG_ERR_UNSUPPORTED_N, nat.MTG_ERR_BAD_DERIVATIVE,
                            nat.MTG_ERR_SIZE_MISMATCH, nat.MTG_ERR_TOO_LARGE)
N_EVEN = "N must be even and in [2, 12]"
N_COLL = "N must be 6, 8, 10 or 12"
R_RANGE = "derivative_to_optimize must be in [0, N/2-1]"
DIMS = "need K >= 1, D >= 1, batch >= 0"
DIMS_COLL = "need K >= 1, batch >= 0"
SOLVE_LDS = "per-trajectory working set exceeds LDS (reduce K or D)"
CAND = "n_candidates must be >= 1"
D3 = "the collision term needs D == 3"
COLL_PARAMS = "need coll_check_time_increment > 0, map_resolution >= 0, grid resolution > 0, grid dimensions >= 1"
INC_TIME = "increment_time must be > 0 and finite"
SOFT_RANGE = "need 0 <= derivative <= min(4, N - 2) and limit > 0"
SOFT_COUNT = "params with 1 <= n_constraints <= 8 are required"
COST_REQ = "vertex_values, times, scales, cost_out are required; grad_out needs fixed_mask"
COLL_REQ = "vertex_values, times, cost_out and grid->distance are required; grad_out needs fixed_mask"
SOFT_REQ = "vertex_values, times and cost_out are required; grad_out needs fixed_mask"
OBJ_REQ = "values, fixed_mask, x, cost_out (objectives 0, 1: times; 1, 2: grid->distance) are required"
OBJ_BIG = "a component's per-trajectory working set exceeds LDS (reduce K), or the batch is too large"
DT = "dt must be > 0 and derivative >= 0"

SIGNATURES = {  # argument names after the context
    "mtg_solve_linear_batch": "N D K r batch values mask times coeffs free n_free cost status flags",
    "mtg_time_sweep_batch": "N D K r batch values mask times C scales cost status flags",
    "mtg_cost_at_times_batch": "N D K r batch values mask times C scales cost grad flags",
    "mtg_collision_cost_batch": "N D K batch values mask times grid coll cost grad collision n_evaluated status flags",
    "mtg_collision_time_gradient_batch": "N D K batch values times grid coll inc grad_t side_cost side_evaluated walked "
                                         "status flags",
    "mtg_soft_constraint_cost_batch": "N D K batch values mask times soft cost grad maxima status flags",
    "mtg_time_jacobian_batch": "N D K r batch values times C scales inc cost jac flags",
    "mtg_objective_batch": "N D K batch values mask times x x_stride params grid coll soft cost grad weighted collision "
                           "state parts status flags",
    "mtg_coefficients_from_vertices_batch": "N D K batch values times coeffs flags",
    "mtg_vertex_derivatives_batch": "N D K batch coeffs times values flags",
    "mtg_min_max_magnitude_batch": "N D K batch coeffs times derivative dims minimum maximum flags",
    "mtg_evaluate_range_batch": "N D K batch coeffs times t0 t1 dt derivative counts offsets out sample_times flags",
    "mtg_evaluate_range_batch_full": "N D K batch coeffs times t0 t1 dt derivative counts offsets total out sample_times "
                                     "capacity flags",
}
ARRAYS = ("values mask times coeffs free n_free cost status scales grad collision n_evaluated grad_t side_cost "
          "side_evaluated walked maxima jac x weighted state minimum maximum counts offsets out sample_times total").split()
ALL_NULL = {k: None for k in ARRAYS}


def _soft(n=2, derivative=1, limit=1.0):
    return nat.SoftConstraintParams(n, (ctypes.c_int32 * 8)(*[derivative] * 8), (ctypes.c_double * 8)(*[limit] * 8), 1.0,
                                    1e12, 0.05)


def _coll(dt=0.1):
    return nat.CollisionParams(dt, 0.2, 1.0, 0.3, 2.0, (ctypes.c_double * 3)(-7, -7, -7), (ctypes.c_double * 3)(7, 7, 7), 1, 0)


def _obj(objective=2, r=4, inc=0.1, soft=1, reserved=0):
    return nat.ObjectiveParams(objective, r, 0.1, 10.0, 1.0, 1.0, inc, soft, 0, 1, reserved, 0.0)


def _table(ptr):
    """(function, overrides of the valid call, return code, mtg_last_error or None: not set by this check).
    ptr: the address of 4 MiB of zeros, passed for every array; no row reaches a kernel or a copy."""
    def sdf(distance=ptr, resolution=2.0, nx=8):
        return nat.SdfGrid(distance, nx, 8, 8, (ctypes.c_double * 3)(-8, -8, -8), resolution, 0.75)
    huge = 1 << 31
    rows = []
    for fn in ("mtg_solve_linear_batch", "mtg_time_sweep_batch", "mtg_cost_at_times_batch", "mtg_time_jacobian_batch"):
        rows += [(fn, dict(N=3), UNS, N_EVEN), (fn, dict(N=14), UNS, N_EVEN), (fn, dict(r=5), BAD, R_RANGE),
                 (fn, dict(r=-1), BAD, R_RANGE), (fn, dict(K=0), SIZE, DIMS), (fn, dict(D=0), SIZE, DIMS),
                 (fn, dict(batch=-1), SIZE, DIMS), (fn, dict(K=100000), BIG, SOLVE_LDS), (fn, dict(D=64), BIG, SOLVE_LDS),
                 (fn, dict(batch=0, **ALL_NULL), 0, None)]
    fn = "mtg_solve_linear_batch"
    rows += [(fn, {k: None}, INV, "values, fixed_mask and times are required") for k in ("values", "mask", "times")]
    fn = "mtg_time_sweep_batch"
    rows += [(fn, dict(C=0), SIZE, CAND)]
    rows += [(fn, {k: None}, INV, "values, fixed_mask, times, scales, cost_out are required")
             for k in ("values", "mask", "times", "scales", "cost")]
    fn = "mtg_cost_at_times_batch"
    rows += [(fn, dict(C=0), SIZE, CAND), (fn, dict(mask=None), INV, COST_REQ),
             # (N = 2, D = 1: the solve's 160 KiB hold K = 2731, the cost tables' 64 KiB do not)
             (fn, dict(N=2, D=1, K=2731, r=0), BIG, "per-trajectory cost tables exceed LDS (reduce K or D)")]
    rows += [(fn, {k: None}, INV, COST_REQ) for k in ("values", "times", "scales", "cost")]
    fn = "mtg_time_jacobian_batch"
    rows += [(fn, dict(C=0), SIZE, CAND), (fn, dict(inc=-0.1), INV, "increment_time must be finite and >= 0"),
             (fn, dict(inc=float("nan")), INV, "increment_time must be finite and >= 0"),
             (fn, dict(inc=float("inf")), INV, "increment_time must be finite and >= 0"),
             # (K = 32: 166016 B of tables per block against 160 KiB; the solve fits)
             (fn, dict(K=32), BIG, "per-block cost tables exceed LDS (reduce K or D)")]
    rows += [(fn, {k: None}, INV, "vertex_values, times, scales, cost_out are required")
             for k in ("values", "times", "scales", "cost")]
    for fn, req, required, big in (
            ("mtg_collision_cost_batch", COLL_REQ, ("values", "times", "cost"),
             "per-trajectory coefficients exceed LDS (reduce K)"),
            ("mtg_collision_time_gradient_batch", "vertex_values, times, grad_t_out and grid->distance are required",
             ("values", "times", "grad_t"), "one trajectory's coefficients and walk records exceed LDS (reduce K)")):
        rows += [(fn, dict(N=4), UNS, N_COLL), (fn, dict(N=7), UNS, N_COLL), (fn, dict(N=14), UNS, N_COLL),
                 (fn, dict(D=2), INV, D3), (fn, dict(K=0), SIZE, DIMS_COLL), (fn, dict(batch=-1), SIZE, DIMS_COLL),
                 (fn, dict(grid=None), INV, "grid and params are required"),
                 (fn, dict(coll=None), INV, "grid and params are required"),
                 (fn, dict(coll=_coll(dt=0.0)), INV, COLL_PARAMS), (fn, dict(grid=sdf(resolution=0.0)), INV, COLL_PARAMS),
                 (fn, dict(grid=sdf(nx=0)), INV, COLL_PARAMS), (fn, dict(batch=0, **ALL_NULL), 0, None),
                 (fn, dict(grid=sdf(distance=None)), INV, req), (fn, dict(K=4096), BIG, big)]
        rows += [(fn, {k: None}, INV, req) for k in required]
    rows += [("mtg_collision_cost_batch", dict(mask=None), INV, COLL_REQ),
             ("mtg_collision_time_gradient_batch", dict(inc=0.0), INV, INC_TIME),
             ("mtg_collision_time_gradient_batch", dict(inc=float("inf")), INV, INC_TIME),
             ("mtg_collision_time_gradient_batch", dict(batch=huge), BIG,
              "one trajectory's coefficients and walk records exceed LDS (reduce K)")]
    fn = "mtg_soft_constraint_cost_batch"
    soft_big = "per-trajectory working set exceeds LDS (reduce K), or batch >= 2^31"
    soft_d = "the soft-constraint term needs 1 <= D <= 4"
    rows += [(fn, dict(N=4), INV, N_COLL), (fn, dict(N=7), INV, N_COLL), (fn, dict(D=0), INV, soft_d),
             (fn, dict(D=5), INV, soft_d), (fn, dict(K=0), SIZE, DIMS_COLL), (fn, dict(batch=-1), SIZE, DIMS_COLL),
             (fn, dict(soft=None), INV, SOFT_COUNT), (fn, dict(soft=_soft(n=0)), INV, SOFT_COUNT),
             (fn, dict(soft=_soft(n=9)), INV, SOFT_COUNT), (fn, dict(soft=_soft(derivative=5)), INV, SOFT_RANGE),
             (fn, dict(soft=_soft(derivative=-1)), INV, SOFT_RANGE), (fn, dict(soft=_soft(limit=0.0)), INV, SOFT_RANGE),
             (fn, dict(batch=0, **ALL_NULL), 0, None),
             (fn, dict(mask=None), INV, SOFT_REQ), (fn, dict(K=4096), BIG, soft_big), (fn, dict(batch=huge), BIG, soft_big)]
    rows += [(fn, {k: None}, INV, SOFT_REQ) for k in ("values", "times", "cost")]
    fn = "mtg_objective_batch"
    rows += [(fn, dict(params=None), INV, "params are required"),
             (fn, dict(params=_obj(objective=3)), INV, "objective not covered (the solve-based objectives are not)"),
             (fn, dict(params=_obj(objective=-1)), INV, "objective not covered (the solve-based objectives are not)"),
             (fn, dict(params=_obj(reserved=1)), INV, "reserved must be 0 (the numerical-gradient switches are not covered)"),
             (fn, dict(N=3), UNS, N_EVEN), (fn, dict(params=_obj(r=5)), BAD, R_RANGE), (fn, dict(K=0), SIZE, DIMS),
             (fn, dict(K=100000), BIG, SOLVE_LDS), (fn, dict(N=4, params=_obj(r=1)), UNS, N_COLL), (fn, dict(D=2), INV, D3),
             (fn, dict(grid=None), INV, "grid and collision params are required"),
             (fn, dict(coll=None), INV, "grid and collision params are required"),
             (fn, dict(coll=_coll(dt=0.0)), INV, COLL_PARAMS), (fn, dict(grid=sdf(resolution=0.0)), INV, COLL_PARAMS),
             (fn, dict(params=_obj(inc=0.0)), INV, INC_TIME),
             (fn, dict(params=_obj(objective=0), D=5), INV, "objective 0 needs 1 <= D <= 4"),
             (fn, dict(soft=None), INV, "soft params are required iff use_soft_constraints"),
             (fn, dict(params=_obj(soft=0)), INV, "soft params are required iff use_soft_constraints"),
             (fn, dict(params=_obj(objective=0, r=1), N=4), INV, "the soft-constraint term needs N >= 6, D <= 4"),
             (fn, dict(soft=_soft(n=0)), INV, "need 1 <= n_constraints <= 8"),
             (fn, dict(soft=_soft(n=9)), INV, "need 1 <= n_constraints <= 8"),
             (fn, dict(soft=_soft(derivative=5)), INV, SOFT_RANGE), (fn, dict(soft=_soft(limit=-1.0)), INV, SOFT_RANGE),
             (fn, dict(x_stride=-1), INV, "x_stride must be >= 0"), (fn, dict(batch=0, **ALL_NULL), 0, None),
             (fn, dict(params=_obj(objective=1), times=None), INV, OBJ_REQ), (fn, dict(grid=sdf(distance=None)), INV, OBJ_REQ),
             (fn, dict(x_stride=1), INV, "x_stride is shorter than the longest row"),  # (a zero mask frees everything)
             (fn, dict(batch=huge, flags=DEV), BIG, OBJ_BIG)]
    rows += [(fn, {k: None}, INV, OBJ_REQ) for k in ("values", "mask", "x", "cost")]
    for fn in ("mtg_coefficients_from_vertices_batch", "mtg_vertex_derivatives_batch"):
        rows += [(fn, dict(N=3), UNS, N_EVEN), (fn, dict(K=0), SIZE, DIMS), (fn, dict(D=0), SIZE, DIMS),
                 (fn, dict(batch=-1), SIZE, DIMS),
                 (fn, dict(K=4096), BIG, "per-trajectory arrays exceed the LDS staging (reduce K or D)"),
                 (fn, dict(batch=0, **ALL_NULL), 0, None)]
        rows += [(fn, {k: None}, INV, "input, times and output are required") for k in ("values", "times", "coeffs")]
    fn = "mtg_min_max_magnitude_batch"
    rows += [(fn, dict(N=3), UNS, N_EVEN), (fn, dict(K=0), SIZE, DIMS), (fn, dict(batch=-1), SIZE, DIMS),
             (fn, dict(K=257), BIG, "K must be <= 256"),
             (fn, dict(derivative=9), BAD, "derivative must be in [0, N-2] (polynomial.cpp:62-65)"),
             (fn, dict(derivative=-1), BAD, "derivative must be in [0, N-2] (polynomial.cpp:62-65)"),
             (fn, dict(dims=8), INV, "dimension_mask out of range"), (fn, dict(D=33), INV, "dimension_mask out of range"),
             (fn, dict(batch=0, **ALL_NULL), 0, None), (fn, dict(coeffs=None), INV, "coeffs and times are required"),
             (fn, dict(times=None), INV, "coeffs and times are required")]
    fn = "mtg_evaluate_range_batch"
    eval_req = "times and counts required; out needs coeffs and offsets"
    rows += [(fn, dict(N=3), UNS, N_EVEN), (fn, dict(K=0), SIZE, DIMS), (fn, dict(batch=-1), SIZE, DIMS),
             (fn, dict(dt=0.0), INV, DT), (fn, dict(derivative=-1), INV, DT), (fn, dict(batch=0, **ALL_NULL), 0, None),
             (fn, dict(times=None), INV, eval_req), (fn, dict(counts=None), INV, eval_req),
             (fn, dict(coeffs=None), INV, eval_req), (fn, dict(offsets=None), INV, eval_req)]
    fn = "mtg_evaluate_range_batch_full"
    full_dims, full_req = "need K >= 1, D >= 1, batch >= 0, capacity >= 0", "coeffs, times, counts, offsets, total and out are required"
    rows += [(fn, dict(N=3), UNS, N_EVEN), (fn, dict(K=0), SIZE, full_dims), (fn, dict(capacity=-1), SIZE, full_dims),
             (fn, dict(dt=0.0), INV, DT), (fn, dict(derivative=-1), INV, DT),
             (fn, dict(batch=0, **ALL_NULL), INV, full_req)]  # (this entry checks its pointers before the empty batch)
    rows += [(fn, {k: None}, INV, full_req) for k in ("coeffs", "times", "counts", "offsets", "total", "out")]
    valid = dict(N=10, D=3, K=2, r=4, batch=1, C=1, inc=0.1, x_stride=64, derivative=1, dims=0, t0=0.0, t1=1.0, dt=0.1,
                 capacity=16, flags=0, grid=sdf(), coll=_coll(), soft=_soft(), params=_obj(), parts=None)
    valid.update({k: ptr for k in ARRAYS})
    return valid, rows


def test_validation_table():
    """Item 5: the return code and the exact mtg_last_error text of every argument check, in the order
    the entries make them, and each entry's MTG_OK for an empty batch with NULL arrays."""
    lib = nat.load()
    zeros = np.zeros(1 << 22, np.uint8)
    valid, rows = _table(zeros.ctypes.data)
    with mtg.Context(0) as ctx:
        h = ctx.handle
        for fn, over, rc, text in rows:
            args = dict(valid)
            args.update(over)
            argv = [ctypes.byref(v) if isinstance(v, ctypes.Structure) else v
                    for v in (args[k] for k in SIGNATURES[fn].split())]
            assert getattr(lib, fn)(None, *argv) == INV, (fn, over, "null context")
            got = getattr(lib, fn)(h, *argv)
            assert got == rc, (fn, over, got, lib.mtg_last_error(h).decode())
            if text is not None:
                assert lib.mtg_last_error(h).decode() == text, (fn, over)
        # mtg_evaluate_range_batch_full's empty batch: the total is written, nothing else
        total = np.full(1, 7, np.int64)
        args = dict(valid, batch=0, total=total.ctypes.data)
        argv = [ctypes.byref(v) if isinstance(v, ctypes.Structure) else v
                for v in (args[k] for k in SIGNATURES["mtg_evaluate_range_batch_full"].split())]
        assert lib.mtg_evaluate_range_batch_full(h, *argv) == 0 and total[0] == 0
        # the multi-device solve: its own checks, then check_shape on the first context
        ctxs = (ctypes.c_void_p * 1)(h.value)
        tail = [valid[k] for k in SIGNATURES["mtg_solve_linear_batch"].split()]
        multi = lib.mtg_solve_linear_batch_multi
        assert multi(None, 1, *tail) == INV and multi(ctypes.addressof(ctxs), 0, *tail) == INV
        null_ctx = (ctypes.c_void_p * 1)(None)
        assert multi(ctypes.addressof(null_ctx), 1, *tail) == INV
        for flags in (DEV, ASYNC):
            assert multi(ctypes.addressof(ctxs), 1, *tail[:-1], flags) == INV
            assert lib.mtg_last_error(h).decode() == "multi-device solves take host arrays and are synchronous"
        assert multi(ctypes.addressof(ctxs), 1, 3, *tail[1:]) == UNS and lib.mtg_last_error(h).decode() == N_EVEN
        assert multi(ctypes.addressof(ctxs), 1, *tail[:4], 0, *[None] * 8, 0) == 0
        assert multi(ctypes.addressof(ctxs), 1, *tail[:5], None, *tail[6:]) == INV
        assert lib.mtg_last_error(h).decode() == "values, fixed_mask and times are required"
        # the context's own entries
        ms, n = ctypes.c_float(0), ctypes.c_int(0)
        assert lib.mtg_last_kernel_ms(h, None) == INV and lib.mtg_last_kernel_ms(None, ctypes.byref(ms)) == INV
        assert lib.mtg_last_kernel_ms(h, ctypes.byref(ms)) == INV and lib.mtg_last_error(h).decode() == "no timed launch yet"
        assert lib.mtg_enable_timing(h, -1) == INV and lib.mtg_enable_timing(None, 1) == INV
        assert lib.mtg_kernel_times(h, None, 1, ctypes.byref(n)) == INV
        assert lib.mtg_kernel_times(h, ctypes.byref(ms), -1, ctypes.byref(n)) == INV
        assert lib.mtg_kernel_times(h, ctypes.byref(ms), 1, None) == INV
        for f in (lib.mtg_synchronize, lib.mtg_reset_stream):
            assert f(None) == INV
        assert lib.mtg_set_stream(None, None) == INV and lib.mtg_get_stream(None) is None
        assert lib.mtg_last_error(None).decode() == "null context"
        assert lib.mtg_debug_fail_next_solve(h, 0) == INV and lib.mtg_debug_fail_next_solve(None, -5) == INV
        assert lib.mtg_debug_fail_next_solve(h, nat.MTG_ERR_HIP) == 0
        assert lib.mtg_solve_linear_batch(h, *tail) == nat.MTG_ERR_HIP  # the injected code, before any launch
        assert lib.mtg_last_error(h).decode() == "injected fault (mtg_debug_fail_next_solve)"
