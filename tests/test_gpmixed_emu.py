"""CPU tier of the mixed-precision exact solves: hssk_kernel_matmul_f32 and the refine, solve and exact-variance calls with the
FP32 inner product on the fiber emulator (tests/emu).  The GPU twin is tests/test_gpmixed_gpu.py; the checks live in
tests/gpmixed_cases.py.  Same cases as the GPU tier, except that the exact variance takes 66 test points (two chunks) and the C++
driver runs at n = 160, as in tests/test_gpsolve_emu.py."""
import os
import subprocess

import pytest

import emu_lib
import gpmixed_cases as GM
from strumpack_amd import hssk as K
from strumpack_amd import kernel as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, LIBNAME, N_CPP = emu_lib.build, "strumpack_amd_emu", "160"


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(LIB())
    yield h
    h.close()


@pytest.fixture(scope="module")
def lib():
    return KM.load(LIB())


@pytest.mark.parametrize("n,nc,d,kern,spread,lam", GM.MATMUL_CASES)
def test_matmul_f32(hk, n, nc, d, kern, spread, lam):
    GM.check_matmul(hk, n, nc, d, kern, spread, lam)


@pytest.mark.parametrize("n,d,kern,spread,splits", GM.ONEHOT_CASES)
def test_matmul_f32_one_hot_columns(hk, n, d, kern, spread, splits):
    GM.check_onehot(hk, n, d, kern, spread, splits)


def test_matmul_f32_both_routes(hk):
    GM.check_both_routes(hk)


def test_matmul_f32_diagonal(hk):
    GM.check_diagonal(hk)


def test_matmul_f32_column_independence(hk):
    GM.check_columns(hk)


def test_matmul_f32_refusals(hk):
    GM.check_refusals(hk)


@pytest.mark.parametrize("kern,d,lam,hscale", GM.REFINE_CASES)
def test_mixed_refine(lib, tmp_path, kern, d, lam, hscale):
    GM.check_refine(KM, lib, kern, d, lam, hscale, str(tmp_path / "m.bin"))


def test_mixed_refine_on_the_matrix_core_route(lib, hk, tmp_path):
    GM.check_refine_matrix_cores(KM, lib, hk, str(tmp_path / "m.bin"))


def test_mixed_refine_spends_fewer_fp64_products(lib):
    GM.check_fewer_fp64_products(KM, lib)


def test_mixed_solve_blocks_and_zero_column(lib, tmp_path):
    GM.check_solve(KM, lib, str(tmp_path / "m.bin"))


@pytest.mark.parametrize("kern,d,lam,hscale", [("gauss", 1, 0.05, 1.0), ("laplace", 8, 0.05, 1.0)])
def test_mixed_exact_variance(lib, kern, d, lam, hscale):
    GM.check_variance(KM, lib, kern, d, lam, hscale, m_test=66)


def test_mixed_fallback(lib, tmp_path):
    GM.check_fallback(KM, lib, str(tmp_path / "m.bin"))


def test_precision_setting(lib):
    GM.check_precision_setting(KM, lib)


def test_mixed_refusals_and_lifecycle(lib):
    GM.check_refusals_and_lifecycle(KM, lib)


def test_cpp_gpmixed_kernel_driver(tmp_path):
    """tests/cpp/test_gpmixed_kernel.cpp: the C++ members in mixed mode against dense algebra on the host"""
    libdir = os.path.dirname(LIB())
    exe = str(tmp_path / "gpmixed_kernel")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "strumpack_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gpmixed_kernel.cpp"), "-o", exe,
                    "-L" + libdir, "-l" + LIBNAME, "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, N_CPP, str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "# exiting" in r.stdout, r.stdout + r.stderr
