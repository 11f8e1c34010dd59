"""CPU tier of the native single-precision sketch: the kernel sources and the host engine on the fiber emulator (tests/emu),
at sizes the emulator finishes in seconds.  The GPU twin is tests/test_f32_gpu.py; the checks live in tests/f32_cases.py."""
import pytest

import emu_lib
import f32_cases as FC
from strumpack_amd import capi
from strumpack_amd import hssk as K


@pytest.fixture(scope="module")
def L():
    return capi.load(emu_lib.build())


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(emu_lib.build())
    yield h
    h.close()


# interior path (whole 64-column tiles, k a multiple of 16, aligned operand), masked path (ragged everything, odd leading
# dimensions, narrow outputs), and K-splits of two and more chunks with both reduce kernels
@pytest.mark.parametrize("m,n,k,tb,alpha,beta,lda_pad,ldb_pad", [
    (192, 128, 64, 1, 1.0, 0.0, 0, 0),
    (192, 128, 64, 0, -1.5, 0.5, 3, 4),
    (64, 200, 48, 1, 1.0, 0.0, 5, 0),
    (130, 77, 50, 1, -0.5, 2.0, 5, 1),
    (130, 77, 50, 0, 1.0, 0.0, 1, 3),
    (200, 65, 50, 0, 1.0, 1.0, 2, 1),
    (16, 64, 16, 1, 2.0, 0.0, 0, 0),
    (7, 3, 1, 0, 1.0, 0.0, 1, 1),
    (64, 128, 1024, 1, 1.0, 0.0, 0, 0),
    (64, 64, 1040, 0, -1.0, 0.5, 5, 0),
    (24, 70, 3001, 1, 1.0, 0.0, 5, 1),
    (32, 5, 13000, 0, 1.0, 0.0, 5, 1),
])
def test_sgemm_sketch(hk, m, n, k, tb, alpha, beta, lda_pad, ldb_pad):
    FC.case_sgemm(hk, m, n, k, tb, alpha=alpha, beta=beta, lda_pad=lda_pad, ldb_pad=ldb_pad)


def test_sgemm_sketch_empty(hk):
    FC.case_sgemm(hk, 8, 9, 0, 1, alpha=1.0, beta=0.5)


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
