"""CPU tier of the gradient of the log marginal likelihood from a kept fit: hssk_kernel_matmul, hssk_coldots and the gradient,
probe and residual calls on the fiber emulator (tests/emu).  The GPU twin is tests/test_gpgrad_gpu.py; the checks live in
tests/gpgrad_cases.py."""
import os
import subprocess

import pytest

import emu_lib
import gpgrad_cases as GG
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


@pytest.mark.parametrize("kern,d", [("gauss", 8), ("laplace", 1)])
def test_oracle_gradient_against_differences(kern, d):
    GG.check_oracle(kern, d)


@pytest.mark.parametrize("n,nc,d,kern,deriv,splits,lam", GG.MATMUL_CASES)
def test_kernel_matmul(hk, n, nc, d, kern, deriv, splits, lam):
    GG.check_matmul(hk, n, nc, d, kern, deriv, splits, lam)


def test_kernel_matmul_properties(hk):
    GG.check_matmul_properties(hk)


def test_kernel_matmul_refusals(hk):
    GG.check_matmul_refusals(hk)


@pytest.mark.parametrize("nc", [1, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_coldots(hk, n, nc):
    GG.check_coldots(hk, n, nc)


@pytest.mark.parametrize("kern,d,lam,hscale", GG.GRADIENT_CASES)
def test_model_gradient(lib, tmp_path, kern, d, lam, hscale):
    GG.check_model_gradient(KM, lib, kern, d, lam, hscale, str(tmp_path / "m.bin"))


def test_exact_trace_and_several_blocks(lib, tmp_path):
    GG.check_exact_trace(KM, lib, str(tmp_path / "m.bin"))


def test_seeded_gradient(lib):
    GG.check_seeded(KM, lib)


@pytest.mark.parametrize("kern,d,lam,hscale", [("gauss", 8, 4.0, 1.0), ("laplace", 8, 0.05, 1.0)])
def test_fit_residual(lib, kern, d, lam, hscale):
    GG.check_fit_residual(KM, lib, kern, d, lam, hscale)


@pytest.mark.parametrize("kern,d,lam1,lam2,hscale", [("gauss", 8, 4.0, 0.05, 0.5), ("laplace", 1, 0.05, 4.0, 1.0)])
def test_gradient_after_set_lambda(lib, tmp_path, kern, d, lam1, lam2, hscale):
    GG.check_after_set_lambda(KM, lib, kern, d, lam1, lam2, hscale, str(tmp_path / "m.bin"))


def test_gradient_refusals_and_lifecycle(lib):
    GG.check_gradient_lifecycle(KM, lib)


def test_cpp_gpgrad_kernel_driver(tmp_path):
    """tests/cpp/test_gpgrad_kernel.cpp: the C++ members of the gradient against dense algebra on the host"""
    libdir = os.path.dirname(LIB())
    exe = str(tmp_path / "gpgrad_kernel")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "strumpack_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gpgrad_kernel.cpp"), "-o", exe,
                    "-L" + libdir, "-l" + LIBNAME, "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, N_CPP], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "# exiting" in r.stdout, r.stdout + r.stderr
