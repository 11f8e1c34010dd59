"""GPU tier of the joint predictive covariance (product library): hssk_kernel_cross_split, hssk_kernel_cross_matmul and the kept model's
predict_covariance / sample_posterior.  The CPU twin is tests/test_gpcov_emu.py; the checks live
in tests/gpcov_cases.py."""
import os
import subprocess

import pytest

import gpcov_cases as GC
from strumpack_amd import _loader
from strumpack_amd import hssk as K
from strumpack_amd import kernel as KM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(_loader.lib_path())
    yield h
    h.close()


@pytest.fixture(scope="module")
def lib():
    return KM.load(_loader.lib_path())


@pytest.mark.parametrize("n,m,d", GC.CROSS_SHAPES)
def test_kernel_cross_split(hk, n, m, d):
    GC.check_cross_split(hk, n, m, d)


def test_kernel_cross_split_refusals(hk):
    GC.check_cross_split_refusals(hk)


@pytest.mark.parametrize("n,m,nc,d,kern,splits", GC.CROSS_MATMUL_CASES)
def test_kernel_cross_matmul(hk, n, m, nc, d, kern, splits):
    GC.check_cross_matmul(hk, n, m, nc, d, kern, splits)


def test_kernel_cross_matmul_properties(hk):
    GC.check_cross_matmul_properties(hk)


def test_kernel_cross_matmul_refusals(hk):
    GC.check_cross_matmul_refusals(hk)


@pytest.mark.parametrize("kern,d,lam,hscale", GC.MODEL_CASES)
def test_model_covariance(lib, tmp_path, kern, d, lam, hscale):
    GC.check_model(KM, lib, kern, d, lam, hscale, str(tmp_path / "m.bin"))


@pytest.mark.parametrize("kern", ["gauss", "laplace"])
def test_exact_covariance(lib, kern):
    GC.check_exact(KM, lib, kern, f32=kern == "gauss")


def test_widths(lib, tmp_path):
    GC.check_widths(KM, lib, str(tmp_path / "m.bin"))


def test_after_set_lambda(lib, tmp_path):
    GC.check_set_lambda(KM, lib, str(tmp_path / "m.bin"))


def test_sample_posterior(lib):
    GC.check_sample_posterior(KM, lib)


def test_refusals(lib):
    GC.check_refusals(KM, lib)


def test_cpp_gpcov_kernel_driver(tmp_path):
    """tests/cpp/test_gpcov_kernel.cpp: the three C++ members against dense algebra on the host"""
    libdir = os.path.dirname(_loader.lib_path())
    exe = str(tmp_path / "gpcov_kernel")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "strumpack_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gpcov_kernel.cpp"), "-o", exe,
                    "-L" + libdir, "-lstrumpack_amd", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, "2000", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "# exiting" in r.stdout, r.stdout + r.stderr
