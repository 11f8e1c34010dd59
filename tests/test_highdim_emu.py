"""CPU tier of kernel ridge regression beyond R^64: the neighbour search, the FP64 and the FP32 prediction sums and the C interface
on the fiber emulator (tests/emu), at sizes the emulator finishes in seconds.  The GPU twin is tests/test_highdim_gpu.py; the
checks live in tests/highdim_cases.py."""
import pytest

import emu_lib
import highdim_cases as HD
from strumpack_amd import hssk as K
from strumpack_amd import kernel as KM


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(emu_lib.build())
    yield h
    h.close()


@pytest.fixture(scope="module")
def lib():
    return KM.load(emu_lib.build())


@pytest.mark.parametrize("n,d,k,lattice", HD.KNN_GENERAL)
def test_knn_beyond_64_coordinates(hk, n, d, k, lattice):
    HD.case_knn_wide(hk, n, d, k, lattice)


@pytest.mark.parametrize("n,d,k,lattice,filtered", HD.KNN_FILTERED)
def test_knn_filtered_beyond_64_coordinates(hk, n, d, k, lattice, filtered):
    HD.case_knn_wide_filtered(hk, n, d, k, lattice, filtered)


def test_knn_filtered_needs_the_slack_of_its_threshold(hk):
    HD.case_knn_filtered_far_from_the_mean(hk)


@pytest.mark.parametrize("n,m,d", HD.PREDICT_WIDE_SHAPES)
def test_kernel_predict_beyond_64_coordinates(hk, n, m, d):
    HD.case_kernel_predict_wide(hk, n, m, d)


@pytest.mark.parametrize("d", HD.F32_WIDE_DIMS)
def test_f32_predict_wide(hk, d):
    HD.case_f32_wide(hk, d)


def test_f32_predict_wide_sentinel(hk):
    HD.case_f32_wide_sentinel(hk)


def test_f32_predict_wide_errors(hk):
    HD.case_f32_wide_errors(hk)


# (n = 400 with leaves of 32: the smallest tree of four levels; the emulator takes the n = 2000 of the GPU tier in minutes.
# Left out of this tier for time: (784, 1e-4), whose four fits pass the 30 s a test may take here, and the two tests against
# the reference's fixture of 1500 points in R^100 (some 20 s each on the emulator, where both pass); all three run in
# tests/test_highdim_gpu.py)
@pytest.mark.parametrize("d,rel_tol", [(100, 1e-2), (100, 1e-4), (784, 1e-2)])
def test_c_api_end_to_end(lib, d, rel_tol):
    HD.case_capi_end_to_end(KM, lib, d, rel_tol, n=400, m=20, leaf=32)
