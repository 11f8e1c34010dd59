"""GPU tier of the native single-precision sketch (product library, FP32 matrix cores): the kernels at the shapes the sketch
meets, the SPX_s_struct_from_dense_device entry against the reference's float fixture and the promoted host path, and one
full-size run.  The CPU twin is tests/test_f32_emu.py; the checks live in tests/f32_cases.py."""
import pytest

import f32_cases as FC
from strumpack_amd import _loader, capi
from strumpack_amd import hssk as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return capi.load(_loader.lib_path())


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(_loader.lib_path())
    yield h
    h.close()


@pytest.mark.parametrize("tb", [1, 0])
@pytest.mark.parametrize("m,n,k,alpha,beta,lda_pad,ldb_pad", [
    (192, 4096, 4096, 1.0, 0.0, 0, 0),
    (64, 1000, 3001, -1.5, 0.5, 5, 1),
    (130, 777, 2050, 1.0, 0.0, 3, 3),
    (200, 65, 50, -0.5, 2.0, 1, 1),
    (16, 64, 16, 2.0, 0.0, 0, 0),
    (192, 33000, 20000, 1.0, 0.0, 0, 0),
    (192, 96, 100000, 1.0, 0.5, 5, 4),
])
def test_sgemm_sketch(hk, m, n, k, tb, alpha, beta, lda_pad, ldb_pad):
    FC.case_sgemm(hk, m, n, k, tb, alpha=alpha, beta=beta, lda_pad=lda_pad, ldb_pad=ldb_pad)


def test_sgemm_sketch_odd_leading_dimension_large(hk):
    # an interior-sized problem whose operand is not aligned: everything through the masked kernel
    FC.case_sgemm(hk, 192, 1024, 2048, 1, alpha=1.0, beta=0.0, lda_pad=1, ldb_pad=3)
    FC.case_sgemm(hk, 192, 1024, 2048, 0, alpha=1.0, beta=0.0, lda_pad=1, ldb_pad=3)


def test_gather_elems_f32(hk):
    FC.case_gather_elems_f32(hk)


def test_narrow_f32(hk):
    FC.case_narrow_f32(hk)


@pytest.mark.parametrize("precision", [1, 2])
def test_reference_float_fixture(L, hk, precision):
    FC.check_fixture(L, hk, precision)


def test_exact_route_equals_promoted_host_path(L, hk):
    FC.check_exact_route_vs_host(L, hk)


def test_auto_rule(L, hk):
    FC.check_auto_rule(L, hk)


def test_errors(L, hk):
    FC.check_errors(L, hk)


def test_tree_pass_serves_float_operand(L, hk):
    FC.check_tree_pass(L, hk)


def test_full_size(L, hk):
    FC.check_full_size(L, hk, n=32768, rel_tol=1e-4, precision=1)
