"""GPU tier of the Matern kernels (types 3 and 4; product library): the FP64 sums, the exact products and the FP32 routes.
The CPU twin is tests/test_matern_emu.py; the checks live in tests/matern_cases.py."""
import pytest

import gp_cases as GP
import matern_cases as MC
from strumpack_amd import _loader
from strumpack_amd import hssk as K

pytestmark = pytest.mark.gpu

LIB = _loader.lib_path


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(LIB())
    yield h
    h.close()


@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("kern", MC.KERNS)
def test_oracle_gradient_against_differences(kern, d):
    MC.check_oracle(kern, d)


@pytest.mark.parametrize("n,m,d", GP.CROSS_SHAPES)
@pytest.mark.parametrize("kern", MC.KERNS)
def test_cross_and_cols(hk, kern, n, m, d):
    MC.check_cross_and_cols(hk, kern, n, m, d)


@pytest.mark.parametrize("n,nc,d,kern,deriv,splits,lam", MC.MATMUL_CASES)
def test_kernel_matmul(hk, n, nc, d, kern, deriv, splits, lam):
    MC.check_matmul(hk, n, nc, d, kern, deriv, splits, lam)


def test_kernel_matmul_properties(hk):
    MC.check_matmul_properties(hk)


@pytest.mark.parametrize("n,nc,d,kern,lam", MC.MATMUL32_CASES)
def test_kernel_matmul_f32(hk, n, nc, d, kern, lam):
    MC.check_matmul32(hk, n, nc, d, kern, lam)


def test_kernel_matmul_f32_properties(hk):
    MC.check_matmul32_properties(hk)


@pytest.mark.parametrize("n,m,d", MC.PREDICT32_CASES)
@pytest.mark.parametrize("kern", MC.KERNS)
def test_predict_f32(hk, kern, n, m, d):
    MC.check_predict32(hk, kern, n, m, d)


def test_predict_f32_refusals(hk):
    MC.check_predict32_refusals(hk)


def test_device_refusals(hk):
    MC.check_refusals(hk)

