"""GPU tier of the single-precision kernel ridge regression path (product library, FP32 matrix cores): hssk_kernel_predict_f32 at
full sizes, the STRUMPACK_*_float entry points pinned to the double ones and to the reference's fixtures, the resident model and
the device entry.  The CPU twin is tests/test_kpredict_emu.py; the checks live in tests/kpredict_cases.py."""
import os
import subprocess

import numpy as np
import pytest

import kpredict_cases as PC
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


@pytest.mark.parametrize("d", [1, 5, 8, 29, 64])
def test_types_and_dimensions(hk, d):
    PC.case_types_and_dimensions(hk, d)
    PC.case_types_and_dimensions(hk, d, n=1500, m=300)


def test_small_and_empty(hk):
    PC.case_small_and_empty(hk)


def test_splits(hk):
    PC.case_splits(hk, [(200, 70, 1), (257, 70, 2), (1500, 70, 6), (100000, 64, 391), (20000, 3000, 44)])


def test_offset(hk):
    PC.case_offset(hk, n=5000, m=700)


def test_bimodal_takes_the_difference_form_only(hk):
    PC.case_bimodal(hk, n=4864, m=1000)     # 76 x 16 tiles


def test_outliers_take_both_routes(hk):
    PC.case_outliers(hk, n=5000, m=900)


def test_uniform_cube_stays_on_the_matrix_cores(hk):
    r = np.random.default_rng(12)
    X, T, w = r.random((10240, 8)), r.random((1000, 8)), r.standard_normal(10240)
    PC.check_predict(hk, X, T, w, 0, 1.3, tag="uniform [0,1]^8", routes="mfma")


def test_errors(hk):
    PC.case_errors(hk)


@pytest.mark.parametrize("tag,inject", [("gauss_400", True), ("gauss_400", False), ("laplace_400", True), ("anova_400", True),
                                        ("gauss_1500", True), ("gauss_1500", False), ("gauss_10k", True)])
def test_float_api_equals_double_api(lib, tag, inject):
    PC.check_float_vs_double(KM, lib, tag, inject)


@pytest.mark.parametrize("tag", ["gauss_400", "laplace_400", "gauss_1500"])
def test_float_api_against_reference_fixture(lib, tag):
    PC.check_float_vs_fixture(KM, lib, tag, *PC.FIXTURE_TOL[tag])


def test_resident_model_and_device_entry(lib):
    PC.check_resident_and_device_entry(KM, lib)


def test_lifecycle(lib):
    PC.check_lifecycle(KM, lib)


def test_double_handle_is_what_it_was(hk):
    import kernel_cases as KC
    KC.case_kernel_predict(hk)


def test_cpp_float_kernel_driver(tmp_path):
    libdir = os.path.dirname(_loader.lib_path())
    exe = str(tmp_path / "float_kernel")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "strumpack_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_float_kernel.cpp"), "-o", exe,
                    "-L" + libdir, "-lstrumpack_amd", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "# exiting" in r.stdout, r.stdout + r.stderr
