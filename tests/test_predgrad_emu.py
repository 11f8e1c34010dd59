"""CPU tier of the gradients of the predicted mean and variance in the test points: hssk_kernel_predict_grad and the kept model's
predict_gradient / predict_variance_gradient on the fiber emulator (tests/emu).  The GPU twin is tests/test_predgrad_gpu.py; the
checks live in tests/predgrad_cases.py.  test_oracle_formulas is numpy only (no library is loaded), so it belongs to this tier
alone and has no twin in the GPU file."""
import os
import subprocess

import pytest

import emu_lib
import predgrad_cases as PG
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


@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("kern", list(PG.TYPES))
def test_oracle_formulas(kern, d):
    """numpy only: the derivative formulas against central differences of the dense mean and variance"""
    PG.check_oracle(kern, d)


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
    libdir = os.path.dirname(emu_lib.build())
    exe = str(tmp_path / "predgrad_kernel")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "strumpack_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_predgrad_kernel.cpp"), "-o", exe,
                    "-L" + libdir, "-lstrumpack_amd_emu", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, "160", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "# exiting" in r.stdout, r.stdout + r.stderr
