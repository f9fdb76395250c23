"""Shared inputs of the ragged vertex-map and collision tests (test_collision_ragged_host.py,
test_gpu_vertex_map_ragged.py, test_gpu_collision_ragged.py): per-K groups of the inputs of
tests/_vertex_map_model.py and of the trajectories of tests/_collision_model.py, their CSR arrays in a
given order, and the comparison against a uniform entry run on every packed K-group."""
import functools

import numpy as np

import mav_trajectory_generation_cmake_amd as mtg
import _collision_model as CM
import _vertex_map_model as VM

KS = (1, 2, 3, 5, 8)


# ---- the vertex maps -----------------------------------------------------------------------------
def groups_of_counts(N, D, seg, seed=0):
    """({K: (x [B_K][K+1][h][D], T [B_K][K], c [B_K][K][D][N])}, order) for a list of segment counts: the
    inputs of _vertex_map_model.inputs per K, and the batch order [(K, index in its group)] that gives the
    trajectories the segment counts `seg`, in that order."""
    seg = [int(k) for k in seg]
    counts = {K: seg.count(K) for K in sorted(set(seg))}
    groups = {K: VM.inputs(N, D, K, n, seed=seed) for K, n in counts.items()}
    seen, order = {}, []
    for K in seg:
        order.append((K, seen.get(K, 0)))
        seen[K] = seen.get(K, 0) + 1
    return groups, order


def shuffled(order, seed=0):
    rng = np.random.default_rng(seed)
    return [order[j] for j in rng.permutation(len(order))]


def same_bytes(have, want, what):
    """assert_array_equal (NaN in the same places) for the message, then every byte."""
    have, want = np.asarray(have), np.asarray(want)
    np.testing.assert_array_equal(have, want, err_msg=what)
    assert np.ascontiguousarray(have).tobytes() == np.ascontiguousarray(want).tobytes(), what


def vertex_csr(groups, order):
    """(x [sum K + B][h][D], T [sum K], c [sum K][D][N], seg_count [B]) of the trajectories in `order`."""
    x = np.ascontiguousarray(np.concatenate([groups[K][0][i] for K, i in order]))
    T = np.ascontiguousarray(np.concatenate([groups[K][1][i] for K, i in order]))
    c = np.ascontiguousarray(np.concatenate([groups[K][2][i] for K, i in order]))
    return x, T, c, np.array([K for K, _ in order], dtype=np.int32)


def per_group(order, call):
    """{K: call(K, indices of the group's members, in batch order)} and, per trajectory of the batch, its
    place in that result."""
    res, place = {}, []
    for K in sorted({K for K, _ in order}):
        idx = [i for k, i in order if k == K]
        res[K] = call(K, idx)
    seen = {}
    for K, _ in order:
        place.append((K, seen.get(K, 0)))
        seen[K] = seen.get(K, 0) + 1
    return res, place


def assert_vertex_maps_equal_the_uniform(order, groups, got_x, got_c, uniform_derivatives, uniform_coefficients,
                                         skip=()):
    """got_x = vertex_derivatives_ragged(c), got_c = coefficients_from_vertices_ragged(x): every trajectory's
    bytes against uniform_derivatives(c [n][K][D][N], T) / uniform_coefficients(N, x [n][V][h][D], T) run on
    its packed K-group.  Trajectories whose K is in `skip` are left to the caller."""
    seg = np.array([K for K, _ in order], dtype=np.int32)
    N = next(iter(groups.values()))[2].shape[-1]
    ks = [K for K in sorted({K for K, _ in order}) if K not in skip]
    sub = [(K, i) for K, i in order if K in ks]
    want_x, place = per_group(sub, lambda K, idx: uniform_derivatives(np.ascontiguousarray(groups[K][2][idx]),
                                                                      np.ascontiguousarray(groups[K][1][idx])))
    want_c, _ = per_group(sub, lambda K, idx: uniform_coefficients(N, np.ascontiguousarray(groups[K][0][idx]),
                                                                   np.ascontiguousarray(groups[K][1][idx])))
    xs = mtg.split_ragged(got_x, seg, "vertex_values")
    cs = mtg.split_ragged(got_c, seg, "coeffs")
    j = 0
    for b, (K, _) in enumerate(order):
        if K in skip:
            continue
        k, at = place[j]
        j += 1
        same_bytes(xs[b], want_x[k][at], "vertex derivatives of trajectory %d (K = %d)" % (b, K))
        same_bytes(cs[b], want_c[k][at], "coefficients of trajectory %d (K = %d)" % (b, K))
    assert j == len(sub)


# ---- the collision cost --------------------------------------------------------------------------
OUTPUTS = ("cost", "grad", "collision", "n_evaluated", "status")


def collision_params(dt=0.1, map_resolution=0.2, continuous=True):
    """The sphere map with the parameters of the issue: dt 0.1, map_resolution 0.2, continuous lookup."""
    grid = CM.maps()["sphere"]
    prm = CM.Params(dt, map_resolution, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, continuous)
    return grid, prm


@functools.lru_cache(maxsize=None)
def collision_groups(N, counts, seed0=0, long_segment=False):
    """{K: (x [B_K][V][h][3], mask [B_K][V], times [B_K][K])} for counts = ((K, B_K), ..): smooth random
    trajectories of _collision_model.random_trajectory with their own segment times in [0.9, 2.6].  With
    long_segment the first K = 2 trajectory gets a segment of 7.33 s: 74 clock samples at dt = 0.1, more
    than one chunk of 64."""
    out = {}
    for K, B in counts:
        rng = np.random.default_rng([seed0, N, K])
        times = rng.uniform(0.9, 2.6, size=(B, K))
        if long_segment and K == 2:
            times[0, 0] = 7.33
        xs, ms = [], []
        for j in range(B):
            x, m = CM.random_trajectory(N, K, seed0 * 10000 + K * 100 + j, times[j])
            xs.append(x)
            ms.append(m)
        out[K] = (np.array(xs), np.array(ms), times)
        for a in out[K]:
            a.setflags(write=False)
    return out


def collision_order(groups, how, seed=0):
    order = [(K, i) for K in sorted(groups) for i in range(groups[K][0].shape[0])]
    return shuffled(order, seed) if how == "shuffled" else order


def collision_csr(groups, order):
    """(x [sum K + B][h][3], mask [sum K + B], times [sum K], seg_count [B]) of the trajectories in `order`."""
    x = np.ascontiguousarray(np.concatenate([groups[K][0][i] for K, i in order]))
    mask = np.ascontiguousarray(np.concatenate([groups[K][1][i] for K, i in order]))
    times = np.ascontiguousarray(np.concatenate([groups[K][2][i] for K, i in order]))
    return x, mask, times, np.array([K for K, _ in order], dtype=np.int32)


def to_host(out):
    return {k: np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def assert_collision_equals_the_uniform(got, order, groups, uniform, grad=True):
    """Every output byte of the ragged result `got`, per trajectory, against uniform(x, times, mask) run on
    its packed K-group (a dict like collision_cost_batch's)."""
    got = to_host(got)
    seg = np.array([K for K, _ in order], dtype=np.int32)
    want, place = per_group(order, lambda K, idx: to_host(uniform(np.ascontiguousarray(groups[K][0][idx]),
                                                                  np.ascontiguousarray(groups[K][2][idx]),
                                                                  np.ascontiguousarray(groups[K][1][idx]))))
    names = [n for n in OUTPUTS if grad or n != "grad"]
    assert sorted(got) == sorted(names)
    views = {n: mtg.split_ragged(got[n], seg, n, D=3) for n in names}
    for b, (K, at) in enumerate(place):
        for n in names:
            have, ref = np.asarray(views[n][b]), np.asarray(want[K][n][at])
            same_bytes(have.reshape(ref.shape), ref, "%s of trajectory %d (K = %d, #%d of its group)" % (n, b, K, at))
