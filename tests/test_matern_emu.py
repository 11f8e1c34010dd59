"""CPU tier of the Matern kernels (types 3 and 4): the FP64 sums, the exact products and the FP32 routes on the fiber emulator
(tests/emu), small shapes only.  The GPU twin is tests/test_matern_gpu.py; the checks live in tests/matern_cases.py."""
import pytest

import emu_lib
import matern_cases as MC
from strumpack_amd import hssk as K

LIB = emu_lib.build


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(LIB())
    yield h
    h.close()


@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("kern", MC.KERNS)
def test_oracle_gradient_against_differences(kern, d):
    MC.check_oracle(kern, d)


@pytest.mark.parametrize("n,m,d", [(130, 130, 1), (130, 65, 64), (70, 130, 70)])
@pytest.mark.parametrize("kern", MC.KERNS)
def test_cross_and_cols(hk, kern, n, m, d):
    MC.check_cross_and_cols(hk, kern, n, m, d)


@pytest.mark.parametrize("n,nc,d,kern,deriv,splits,lam", MC.MATMUL_CASES)
def test_kernel_matmul(hk, n, nc, d, kern, deriv, splits, lam):
    MC.check_matmul(hk, n, nc, d, kern, deriv, splits, lam)


def test_kernel_matmul_properties(hk):
    MC.check_matmul_properties(hk)


@pytest.mark.parametrize("n,nc,d,kern,lam", MC.MATMUL32_CASES[:6])
def test_kernel_matmul_f32(hk, n, nc, d, kern, lam):
    MC.check_matmul32(hk, n, nc, d, kern, lam)


def test_kernel_matmul_f32_properties(hk):
    MC.check_matmul32_properties(hk)


@pytest.mark.parametrize("n,m,d", [c for c in MC.PREDICT32_CASES if c[0] * c[1] <= 130 * 70])
@pytest.mark.parametrize("kern", MC.KERNS)
def test_predict_f32(hk, kern, n, m, d):
    MC.check_predict32(hk, kern, n, m, d)


def test_predict_f32_refusals(hk):
    MC.check_predict32_refusals(hk)


def test_device_refusals(hk):
    MC.check_refusals(hk)

