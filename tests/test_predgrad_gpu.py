"""GPU tier of the gradients of the predicted mean and variance in the test points (product library): hssk_kernel_predict_grad and
the kept model's predict_gradient / predict_variance_gradient.  The CPU twin is tests/test_predgrad_emu.py; the checks live in
tests/predgrad_cases.py."""
import os
import subprocess

import pytest

import predgrad_cases as PG
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


@pytest.mark.parametrize("n,m,d", PG.GRAD_SHAPES)
def test_kernel_predict_grad(hk, n, m, d):
    PG.check_predict_grad(hk, n, m, d)


def test_kernel_predict_grad_exact_zeros(hk):
    PG.check_exact_zeros(hk)


def test_kernel_predict_grad_refusals(hk):
    PG.check_grad_refusals(hk)


@pytest.mark.parametrize("kern,d,lam,hscale", PG.MODEL_CASES)
def test_model_gradients(lib, tmp_path, kern, d, lam, hscale):
    PG.check_model(KM, lib, kern, d, lam, hscale, str(tmp_path / "m.bin"))


def test_exact_variance_gradient(lib):
    PG.check_exact(KM, lib)


def test_widths(lib):
    PG.check_widths(KM, lib)


def test_refusals(lib):
    PG.check_refusals(KM, lib)


def test_cpp_predgrad_kernel_driver(tmp_path):
    """tests/cpp/test_predgrad_kernel.cpp: the three C++ members against dense algebra on the host"""
    libdir = os.path.dirname(_loader.lib_path())
    exe = str(tmp_path / "predgrad_kernel")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "strumpack_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_predgrad_kernel.cpp"), "-o", exe,
                    "-L" + libdir, "-lstrumpack_amd", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, "2000", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "# exiting" in r.stdout, r.stdout + r.stderr
