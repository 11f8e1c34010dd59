"""CPU tier of the single-precision kernel ridge regression path: hssk_kernel_predict_f32 and the STRUMPACK_*_float entry points
on the fiber emulator (tests/emu), at sizes the emulator finishes in seconds.  The GPU twin is tests/test_kpredict_gpu.py; the
checks live in tests/kpredict_cases.py."""
import os
import subprocess

import pytest

import emu_lib
import kpredict_cases as PC
from strumpack_amd import hssk as K
from strumpack_amd import kernel as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(emu_lib.build())
    yield h
    h.close()


@pytest.fixture(scope="module")
def lib():
    return KM.load(emu_lib.build())


@pytest.mark.parametrize("d", [1, 5, 8, 29, 64])
def test_types_and_dimensions(hk, d):
    PC.case_types_and_dimensions(hk, d)


def test_small_and_empty(hk):
    PC.case_small_and_empty(hk)


def test_splits(hk):
    PC.case_splits(hk, [(200, 70, 1), (257, 70, 2), (1500, 70, 6)])


def test_offset(hk):
    PC.case_offset(hk)


def test_bimodal_takes_the_difference_form_only(hk):
    PC.case_bimodal(hk)


def test_outliers_take_both_routes(hk):
    PC.case_outliers(hk)


def test_errors(hk):
    PC.case_errors(hk)


@pytest.mark.parametrize("tag,inject", [("gauss_400", True), ("gauss_400", False), ("laplace_400", True), ("anova_400", True)])
def test_float_api_equals_double_api(lib, tag, inject):
    PC.check_float_vs_double(KM, lib, tag, inject)


@pytest.mark.parametrize("tag", ["gauss_400", "laplace_400"])
def test_float_api_against_reference_fixture(lib, tag):
    PC.check_float_vs_fixture(KM, lib, tag, *PC.FIXTURE_TOL[tag])


def test_lifecycle(lib):
    PC.check_lifecycle(KM, lib)


def test_cpp_float_kernel_driver(tmp_path):
    """tests/cpp/test_float_kernel.cpp: Kernel<float> through create_kernel<float>, fit and predict, and a user-defined
    subclass predicting on the host, linked against the emulator library"""
    libdir = os.path.dirname(emu_lib.build())
    exe = str(tmp_path / "float_kernel_emu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "strumpack_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_float_kernel.cpp"), "-o", exe,
                    "-L" + libdir, "-lstrumpack_amd_emu", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "# exiting" in r.stdout, r.stdout + r.stderr
