"""GPU tier of kernel ridge regression beyond R^64 (product library): the neighbour search, the FP64 and the FP32 prediction sums
and the C interface at 100 and 784 coordinates.  The CPU twin is tests/test_highdim_emu.py; the checks live in
tests/highdim_cases.py."""
import pytest

import highdim_cases as HD
from strumpack_amd import _loader
from strumpack_amd import hssk as K
from strumpack_amd import kernel as KM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(_loader.lib_path())
    yield h
    h.close()


@pytest.fixture(scope="module")
def lib():
    return KM.load(_loader.lib_path())


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


# (a test per kernel: the FP64 reference of 1500 x 300 pairs in R^784 is what takes the time)
@pytest.mark.parametrize("kind", range(6))
@pytest.mark.parametrize("d", HD.F32_WIDE_DIMS)
def test_f32_predict_wide_several_splits(hk, d, kind):
    HD.case_f32_wide(hk, d, n=1500, m=300, kinds=HD.f32_kinds(d)[kind:kind + 1])


def test_f32_predict_wide_sentinel(hk):
    HD.case_f32_wide_sentinel(hk)


def test_f32_predict_wide_errors(hk):
    HD.case_f32_wide_errors(hk)


@pytest.mark.parametrize("d,rel_tol", [(100, 1e-2), (100, 1e-4), (784, 1e-2), (784, 1e-4)])
def test_c_api_end_to_end(lib, d, rel_tol):
    HD.case_capi_end_to_end(KM, lib, d, rel_tol, n=2000, m=20, leaf=128, device=True)



def test_reference_fixture_with_reference_neighbour_search(lib):
    """--hss_neighbor_search ann in R^100: the reference's pipeline from the raw points -- its permutation, per-node ranks (one off on
    at most 10 % of the nodes), weights to 1e-6"""
    HD.case_reference_fixture(KM, lib, ann=True)


def test_reference_fixture_with_device_neighbours(lib):
    """the exact search beyond R^64 on the same points: the allowances of test_kernel_gpu.test_regression_with_device_neighbours"""
    HD.case_reference_fixture(KM, lib, ann=False)
