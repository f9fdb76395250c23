"""Shared inputs of the ragged-solve tests (test_ragged_host.py, test_gpu_ragged.py): per-K batches from
the reference generators, interleaved into the CSR layout by pack_ragged."""
import numpy as np

import mav_trajectory_generation_cmake_amd as mtg
from _util import off_pattern_batch

OUTPUTS = ("coeffs", "free", "n_free", "cost", "status")


def per_k_batches(N, D, counts, seed0=1, kinds=None):
    """{K: (values [B_K][K+1][N/2][D], mask, times)} for counts = {K: B_K}; kinds = {K: off-pattern kind}
    takes that group's masks from tests/_util.off_pattern_batch, the others are the bench generator's."""
    out = {}
    for i, (K, B) in enumerate(sorted(counts.items())):
        kind = (kinds or {}).get(K)
        if kind:
            out[K] = off_pattern_batch(N, D, K, B, seed0 + 1000 * i, kind)
        else:
            out[K] = mtg.random_vertices_path_batch(N, D, K, B, seed0=seed0 + 1000 * i, max_derivative=min(4, N // 2 - 1))
    return out


def order_of(batches, how, seed=0):
    """A batch order as a list of (K, index in the K-batch): "sorted" by K, or "shuffled"."""
    order = [(K, i) for K in sorted(batches) for i in range(batches[K][0].shape[0])]
    if how == "shuffled":
        rng = np.random.default_rng(seed)
        order = [order[j] for j in rng.permutation(len(order))]
    return order


def ragged_of(batches, order):
    """(values, mask, times, seg_count) CSR arrays of the trajectories in `order`."""
    return mtg.pack_ragged([(batches[K][0][i], batches[K][1][i], batches[K][2][i]) for K, i in order])


def views_of(out, seg_count, D):
    """{name: per-trajectory views} of a ragged result dict (device tensors are brought to the host)."""
    return {k: mtg.split_ragged(v.cpu().numpy() if hasattr(v, "cpu") else v, seg_count, k, D=D) for k, v in out.items()}


def assert_matches_groups(out, seg_count, D, order, reference):
    """Every output of the ragged result equals, per trajectory, reference[K][name][i] (the uniform solve
    of that trajectory's K-group)."""
    got = views_of(out, seg_count, D)
    for name, per_traj in got.items():
        for b, (K, i) in enumerate(order):
            want = reference[K][name][i]
            have = np.asarray(per_traj[b])
            np.testing.assert_array_equal(have, np.asarray(want).reshape(have.shape),
                                          err_msg="%s of trajectory %d (K = %d, #%d of its group)" % (name, b, K, i))
