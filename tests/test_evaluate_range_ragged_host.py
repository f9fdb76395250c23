"""CPU checks of the ragged evaluateRange entries (mtg_evaluate_range_ragged_batch[_full]): the symbols
are exported, declared and prototyped; evaluate_range_capacity on CSR times bounds the oracle's counts;
the ragged kernels cross-compiled for gfx950 contain no contracted Horner step."""
import re
import subprocess

import numpy as np

from mav_trajectory_generation_cmake_amd import _native as nat
from mav_trajectory_generation_cmake_amd.solver import evaluate_range_capacity

ENTRIES = ("mtg_evaluate_range_ragged_batch", "mtg_evaluate_range_ragged_batch_full")


def test_entries_are_exported_declared_and_prototyped():
    header = re.sub(r"/\*.*?\*/", "", open(nat.HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    lib = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in exported, name
        assert name in nat.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None, name
    assert len(lib.mtg_evaluate_range_ragged_batch.argtypes) == 16
    assert len(lib.mtg_evaluate_range_ragged_batch_full.argtypes) == 18
    assert lib.mtg_abi_version() == 5


def test_capacity_helper_bounds_the_oracle_on_csr_times():
    """The inputs of the GPU suite's case 1 (B = 65, K_b from {1, 2, 3, 5, 8, 13}, times in [0.3, 1.5],
    dt = 0.01), open-ended and with t_end inside the trajectories: per trajectory and summed, the bound is
    at least the oracle's count, and it is the uniform helper's bound on each trajectory alone."""
    from oracle import pyoracle
    rng = np.random.default_rng(11)
    Ks = rng.choice([1, 2, 3, 5, 8, 13], size=65)
    Ks[[0, 31, 32, 64]] = 1
    tl = [rng.uniform(0.3, 1.5, int(K)) for K in Ks]
    times = np.concatenate(tl)
    for ts, te in ((0.0, 1e9), (0.0, 2.5), (0.4, 3.0)):
        counts = [pyoracle.evaluate_range(np.zeros((len(t), 1, 2)), t, ts, te, 0.01, 0, max_samples=0)[2] for t in tl]
        per = [evaluate_range_capacity(t, ts, te, 0.01, seg_count=[len(t)]) for t in tl]
        assert all(p >= c for p, c in zip(per, counts))
        assert per == [evaluate_range_capacity(t[None, :], ts, te, 0.01) for t in tl]
        total = evaluate_range_capacity(times, ts, te, 0.01, seg_count=Ks)
        assert total == sum(per) >= sum(counts) > 0
    assert evaluate_range_capacity(np.zeros(0), 0.0, 1.0, 0.01, seg_count=[]) == 0


def test_ragged_evaluate_range_has_no_fma(tmp_path):
    """tests/test_build.py's check on mtg_eval.hip, for the CSR unit: the ragged range kernels contain no
    f64 FMA other than the compiler's f64 -> int64 conversion idiom (constant 0xc1f00000)."""
    import pytest
    import test_build as tb
    if not tb.os.path.exists(tb.hipcc):
        pytest.skip("hipcc not available")
    asm = tb._device_asm("mtg_eval_ragged.hip", tmp_path)
    bodies = tb._kernel_bodies(asm, r"_ZN3mtg17eval_range_kernel")
    assert len(bodies) == 108 and all("Lb1E" in name for name in bodies)  # N x derivative x (D = 3, ST, run-time D), Ragged
    pc = tb._kernel_bodies(asm, r"_ZN3mtg20eval_range_pc_kernel")
    assert len(pc) == 36
    bodies.update(pc)
    for name, body in bodies.items():
        bad = [ln for ln in body.splitlines() if re.search(r"v_fmac?_f64", ln) and "0xc1f00000" not in ln]
        assert not bad, (name, bad[:3])
    # the unit holds the ragged kernels only: the uniform ones stay in mtg_eval.hip
    assert not re.search(r"^_ZN3mtg1[67]eval_(count|runs)_kernelILb[01]ELb0E", asm, flags=re.M)
    assert "eval_scan_kernel" not in asm
