"""tests/cpp/test_collision_ragged.cpp (built under MTG_BUILD_TESTS): the free vertexDerivativesRagged<10>,
coefficientsFromVerticesRagged<10> and collisionCostRagged<10> of the C++ drop-in equal the uniform entries
called per trajectory, bit for bit, on the host policy and -- marked gpu -- through the kernels
(ExecutionPolicy::kDevice) and the batch object's members."""
import os
import shutil
import subprocess

import pytest

from mav_trajectory_generation_cmake_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_entries_equal_the_uniform_ones_on_the_host():
    from test_cpp_api import _cmake_build
    _cmake_build()
    exe = os.path.join(ROOT, "build", "test_collision_ragged")
    assert os.path.exists(exe)
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


@pytest.mark.gpu
def test_ragged_entries_equal_the_uniform_ones_on_the_device(tmp_path, gpu_ctx):
    """Built with g++ against the library in the tree, as test_cpp_api_on_gpu."""
    cxx = shutil.which("g++") or "g++"
    exe = str(tmp_path / "test_collision_ragged")
    libdir = os.path.dirname(nat.LIB_PATH)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-DMTG_CPP_THROW=1", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_collision_ragged.cpp"),
                    "-o", exe, "-L", libdir, "-lmav_trajectory_generation", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
