"""CPU tier of the log-determinant of a factored HSS matrix: hssk_logabsdet_vbatched and SPX_d_struct_logabsdet on the fiber
emulator (tests/emu).  The GPU twin is tests/test_gp_gpu.py; the checks live in tests/gp_cases.py."""
import os
import subprocess

import pytest

import emu_lib
import gp_cases as GP
from strumpack_amd import capi
from strumpack_amd import hssk as K
from strumpack_amd import kernel as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(emu_lib.build())
    yield h
    h.close()


@pytest.fixture(scope="module")
def L():
    return capi.load(emu_lib.build())


@pytest.fixture(scope="module")
def lib():
    return KM.load(emu_lib.build())


def test_logabsdet_kernel(hk):
    GP.check_logabsdet_kernel(hk)


@pytest.mark.parametrize("kind", ["toeplitz", "unsym"])
@pytest.mark.parametrize("name", GP.LOGDET_CASES)
def test_logabsdet(L, tmp_path, name, kind):
    GP.check_logdet(L, name, kind, str(tmp_path / "h.bin"))


@pytest.mark.parametrize("kind", ["toeplitz", "unsym"])
def test_logabsdet_after_shift_and_refactor(L, tmp_path, kind):
    # -1.0: the case as specified (3.7 T stays definite there: its smallest eigenvalue is 1.4); -5.0 on top makes it indefinite
    GP.check_logdet(L, "fused_inner_levels", kind, str(tmp_path / "h.bin"), shifts=(-1.0, -5.0))


def test_logabsdet_nodes_with_nothing_to_eliminate(L, tmp_path):
    GP.check_logdet(L, "nothing_to_eliminate", "full_rank", str(tmp_path / "h.bin"))


def test_logabsdet_refusals(L):
    GP.check_logdet_errors(L)


@pytest.mark.parametrize("n,m,d", GP.CROSS_SHAPES)
def test_kernel_cross_and_predict_cols(hk, n, m, d):
    GP.check_cross_and_cols(hk, n, m, d)


@pytest.mark.parametrize("kern,d,lam,hscale", GP.MODEL_CASES)
def test_kept_model(lib, tmp_path, kern, d, lam, hscale):
    # (the Gauss R^8 fit at lambda = 4 also answers for 1, 64 and 65 test points: one chunk, a full one, a full one and a rest)
    GP.check_model(KM, lib, kern, d, lam, hscale, str(tmp_path / "m.bin"), extra_m=(1, 64, 65) if (kern, d, lam) == ("gauss", 8, 4.0) else ())


@pytest.mark.parametrize("kern,d,lam1,lam2,hscale", [("gauss", 8, 4.0, 0.05, 0.5), ("laplace", 1, 0.05, 4.0, 1.0)])
def test_set_lambda(lib, tmp_path, kern, d, lam1, lam2, hscale):
    GP.check_set_lambda(KM, lib, kern, d, lam1, lam2, hscale, str(tmp_path / "m.bin"))


def test_model_lifecycle(lib, tmp_path):
    GP.check_model_lifecycle(KM, lib, str(tmp_path / "m.bin"))


def test_cpp_gp_kernel_driver(tmp_path):
    """tests/cpp/test_gp_kernel.cpp: the C++ members of the kept model and HSSMatrix::logabsdet end to end against dense algebra
    on the host"""
    libdir = os.path.dirname(emu_lib.build())
    exe = str(tmp_path / "gp_kernel")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "strumpack_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gp_kernel.cpp"), "-o", exe,
                    "-L" + libdir, "-lstrumpack_amd_emu", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe, "160", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "# exiting" in r.stdout, r.stdout + r.stderr
