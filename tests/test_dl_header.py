"""The DL solve kernel's hot kernarg header (csrc/mtg_solve_dl.inc DlHot, filled by dl_fill_hot in the
launcher) against a plain restatement: the four data pointers, the byte sizes of a full wave's
regions, the trajectories per wave, the flags and the last wave's place and trajectory count.
Host only: the library's test hook fills the header for given arguments without launching anything."""
import ctypes
import struct

import pytest

from mav_trajectory_generation_cmake_amd import _native as nat

K_OF = {10: 10, 12: 20}                 # the chain length the kernel is built for, per N
PLAIN, COEFFS, OPTIONAL = 1, 2, 4       # DlHotFlags
FIELDS = ("values", "mask", "times", "coeffs", "vbytes", "mbytes", "tbytes", "obytes", "tpw", "flags", "last_block",
          "last_nvt")
PTRS = dict(values=0x7F0000001000, mask=0x7F0000200000, times=0x7F0000300008, coeffs=0x7F0000400010)


def _hook():
    fn = nat.load().mtgtest_dl_hot_header
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                                 ctypes.c_void_p]
    return fn


def _filled(N, D, K, r, B, n_cand=1, scales=None, optional=False, coeffs=PTRS["coeffs"]):
    buf = (ctypes.c_uint64 * 8)()
    rc = _hook()(N, D, K, r, PTRS["values"], PTRS["mask"], PTRS["times"], coeffs, scales, B, n_cand, int(optional), buf)
    return rc, dict(zip(FIELDS, struct.unpack("<4Q4IiIIi", bytes(buf))))


def _restated(N, D, K, B, n_cand=1, scales=None, optional=False, coeffs=PTRS["coeffs"]):
    V, h = K + 1, N // 2
    tpw = 64 // (2 * D)                 # one lane per (chain, dimension), two chains per trajectory
    blocks = -(-B // tpw)
    return dict(values=PTRS["values"], mask=PTRS["mask"], times=PTRS["times"], coeffs=coeffs or 0,
                vbytes=tpw * V * h * D * 8, mbytes=tpw * V, tbytes=tpw * K * 8, obytes=tpw * K * D * N * 8, tpw=tpw,
                flags=(PLAIN if n_cand == 1 and not scales else 0) | (COEFFS if coeffs else 0) |
                (OPTIONAL if optional else 0),
                last_block=blocks - 1, last_nvt=B - (blocks - 1) * tpw)


@pytest.mark.parametrize("N", [10, 12])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_header_matches_restatement(N, D):
    K = K_OF[N]
    tpw = 64 // (2 * D)
    for B in (1, 9, 10, 11, 23, tpw - 1, tpw, tpw + 1, 10000, 125000, (1 << 31) + 5):
        if B < 1:
            continue
        rc, got = _filled(N, D, K, 3, B)
        assert rc == 0
        assert got == _restated(N, D, K, B), (N, D, B)
        assert 1 <= got["last_nvt"] <= tpw and got["last_block"] * tpw + got["last_nvt"] == B


def test_header_flags():
    N, D, K, B = 10, 3, 10, 33
    for n_cand, scales, optional, coeffs in [(1, None, False, PTRS["coeffs"]), (1, None, True, PTRS["coeffs"]),
                                             (1, None, True, None), (3, 0x7F0000500000, True, None),
                                             (1, 0x7F0000500000, False, PTRS["coeffs"]), (3, None, False, PTRS["coeffs"])]:
        rc, got = _filled(N, D, K, 4, B * n_cand, n_cand, scales, optional, coeffs)
        assert rc == 0
        assert got == _restated(N, D, K, B * n_cand, n_cand, scales, optional, coeffs), (n_cand, scales, optional, coeffs)
    assert _filled(N, D, K, 4, B)[1]["flags"] == PLAIN | COEFFS


def test_header_rejects_shapes_the_kernel_does_not_serve():
    assert _filled(10, 3, 12, 4, 5)[0] == -1    # K is not the kernel's chain length
    assert _filled(8, 3, 10, 3, 5)[0] == -1     # N
    assert _filled(10, 5, 10, 4, 5)[0] == -1    # D
    assert _filled(10, 3, 10, 4, 0)[0] == -1    # an empty batch launches nothing
