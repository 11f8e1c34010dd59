"""GPU tier of the per-coordinate length-scale gradient (automatic relevance determination; product library):
hssk_kernel_matmul_coord, the coordinate gradient of a kept fit and the widths convenience.  The CPU twin is
tests/test_gpard_emu.py; the checks live in tests/gpard_cases.py.  The C++ driver runs at n = 400."""
import os
import subprocess

import pytest

import gpard_cases as GA
from strumpack_amd import _loader
from strumpack_amd import hssk as K
from strumpack_amd import kernel as KM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, LIBNAME, N_CPP = _loader.lib_path, "strumpack_amd", "400"


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(LIB())
    yield h
    h.close()


@pytest.fixture(scope="module")
def lib():
    return KM.load(LIB())


@pytest.mark.parametrize("n,nc,d,kern,splits", GA.COORD_CASES)
def test_kernel_matmul_coord(hk, n, nc, d, kern, splits):
    GA.check_coord(hk, n, nc, d, kern, splits)


def test_kernel_matmul_coord_entries(hk):
    GA.check_entries(hk)


def test_kernel_matmul_coord_properties(hk):
    GA.check_properties(hk)


def test_kernel_matmul_coord_refusals(hk):
    GA.check_refusals(hk)


@pytest.mark.parametrize("kern,d,lam,hscale", GA.MODEL_CASES)
def test_coordinate_gradient(lib, tmp_path, kern, d, lam, hscale):
    """63 probes (one block with alpha) and 70 (two blocks) on one kept fit"""
    GA.check_model_gradient(KM, lib, kern, d, lam, hscale, str(tmp_path / "m.bin"))


def test_coordinate_gradient_seeded(lib):
    GA.check_seeded(KM, lib)


def test_coordinate_gradient_refusals_and_lifecycle(lib):
    GA.check_lifecycle(KM, lib)


def test_widths(lib):
    GA.check_widths(KM, lib)


def test_cpp_gpard_kernel_driver(tmp_path):
    """tests/cpp/test_gpard_kernel.cpp: the C++ members against dense algebra on the host, and the C entry point bit for bit"""
    libdir = os.path.dirname(LIB())
    exe = str(tmp_path / "gpard_kernel")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "strumpack_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gpard_kernel.cpp"), "-o", exe,
                    "-L" + libdir, "-l" + LIBNAME, "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, N_CPP, str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "# exiting" in r.stdout, r.stdout + r.stderr
