"""GPU tier of the solves with the exact kernel matrix from a kept fit (product library): hssk_krylov_start / _orth / _combine and
the refine, solve and exact-variance calls.  The CPU twin is tests/test_gpsolve_emu.py; the checks live in tests/gpsolve_cases.py."""
import os
import subprocess

import pytest

import gpsolve_cases as GS
from strumpack_amd import _loader
from strumpack_amd import hssk as K
from strumpack_amd import kernel as KM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, LIBNAME, N_CPP = _loader.lib_path, "strumpack_amd", "1000"


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(LIB())
    yield h
    h.close()


@pytest.fixture(scope="module")
def lib():
    return KM.load(LIB())


@pytest.mark.parametrize("n,nc,k", GS.ORTH_CASES)
def test_krylov_orth(hk, n, nc, k):
    GS.check_orth(hk, n, nc, k)


@pytest.mark.parametrize("n,nc", GS.START_CASES)
def test_krylov_start(hk, n, nc):
    GS.check_start(hk, n, nc)


@pytest.mark.parametrize("n,nc,kcount", GS.COMBINE_CASES)
def test_krylov_combine(hk, n, nc, kcount):
    GS.check_combine(hk, n, nc, kcount)


def test_krylov_refusals(hk):
    GS.check_krylov_refusals(hk)


@pytest.mark.parametrize("kern,d,lam,hscale,restart", GS.REFINE_CASES)
def test_refine(lib, tmp_path, kern, d, lam, hscale, restart):
    GS.check_refine(KM, lib, kern, d, lam, hscale, restart, str(tmp_path / "m.bin"))


def test_refine_that_does_not_converge(lib):
    GS.check_no_convergence(KM, lib)


def test_solve_blocks_and_zero_column(lib, tmp_path):
    GS.check_solve(KM, lib, str(tmp_path / "m.bin"))


def test_refine_after_set_lambda(lib, tmp_path):
    GS.check_after_set_lambda(KM, lib, str(tmp_path / "m.bin"))


def test_solve_refusals_and_lifecycle(lib):
    GS.check_solve_lifecycle(KM, lib)


@pytest.mark.parametrize("kern,d,lam,hscale", GS.VARIANCE_CASES)
def test_exact_variance(lib, kern, d, lam, hscale):
    GS.check_variance_exact(KM, lib, kern, d, lam, hscale)


def test_cpp_gpsolve_kernel_driver(tmp_path):
    """tests/cpp/test_gpsolve_kernel.cpp: the C++ members against dense algebra on the host"""
    libdir = os.path.dirname(LIB())
    exe = str(tmp_path / "gpsolve_kernel")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "strumpack_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gpsolve_kernel.cpp"), "-o", exe,
                    "-L" + libdir, "-l" + LIBNAME, "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, N_CPP, str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "# exiting" in r.stdout, r.stdout + r.stderr
