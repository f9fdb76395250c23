"""tests/cpp/test_evaluate_range_ragged.cpp (built under MTG_BUILD_TESTS): the batch object's
evaluateRangeRaggedCounts and evaluateRangeRagged equal Trajectory::evaluateRange called per trajectory on
the host policy, bit for bit.  Without a GPU: it builds (-Wall -Wextra -Werror); marked gpu: it runs."""
import os
import shutil
import subprocess

import pytest

from mav_trajectory_generation_cmake_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_evaluate_range_members_build():
    from test_cpp_api import _cmake_build
    _cmake_build()
    assert os.path.exists(os.path.join(ROOT, "build", "test_evaluate_range_ragged"))


@pytest.mark.gpu
def test_ragged_evaluate_range_members_equal_the_trajectory_method(tmp_path, gpu_ctx):
    """Built with g++ against the library in the tree, as test_cpp_api_on_gpu."""
    cxx = shutil.which("g++") or "g++"
    exe = str(tmp_path / "test_evaluate_range_ragged")
    libdir = os.path.dirname(nat.LIB_PATH)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-DMTG_CPP_THROW=1", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_evaluate_range_ragged.cpp"),
                    "-o", exe, "-L", libdir, "-lmav_trajectory_generation", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
