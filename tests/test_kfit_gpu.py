"""GPU tier of the kernel ridge regression fit at high ranks and after neighbour doubling (product library).  The CPU twin is
tests/test_kfit_emu.py; the checks and the cases live in tests/kfit_cases.py.  The small cases lower HSSK_KNN_FILTER_MIN to 600,
so that their rounds of up to 128 neighbours take the filtered search; the 9000-point case runs at the default."""
import pytest

import kfit_cases as KF
from strumpack_amd import _loader
from strumpack_amd import capi
from strumpack_amd import dist as sdist
from strumpack_amd import hssk as K
from strumpack_amd import kernel as KM

pytestmark = pytest.mark.gpu

ENV = {"HSSK_KNN_FILTER_MIN": "600"}
LIB_EXPR = "from strumpack_amd import _loader; path = _loader.lib_path()"
DENSE_CASES = ["A", "B128s", "B128", "B256"]
CASES = DENSE_CASES + ["B9000"]
B_CASES = ["B128s", "B128", "B256", "B9000"]


@pytest.fixture(scope="module")
def lib():
    yield KM.load(_loader.lib_path())
    KF.release()


@pytest.fixture(scope="module")
def L():
    return capi.load(_loader.lib_path())


@pytest.fixture(scope="module")
def hk():
    h = K.Hssk(_loader.lib_path())
    yield h
    h.close()


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    return str(tmp_path_factory.mktemp("kfit") / "model.bin")


def F(lib, name, path):
    return KF.fitted(KM, lib, name, {} if name == "B9000" else ENV, path)


@pytest.mark.parametrize("name", CASES)
def test_regime_and_route_counters(lib, model_path, name):
    base = F(lib, "A_gauss", model_path) if name == "A" else None
    KF.check_regime(F(lib, name, model_path), base)
    KF.check_counters(F(lib, name, model_path), lib)
    if base is not None:
        KF.check_counters(base, lib)


@pytest.mark.parametrize("name", DENSE_CASES + ["A_gauss"])
def test_dense_form_and_solve(lib, model_path, name):
    KF.check_dense(F(lib, name, model_path), lib)


@pytest.mark.parametrize("name", CASES + ["A_gauss"])
def test_second_route_same_answer(lib, model_path, tmp_path, name):
    KF.check_second_route(F(lib, name, model_path), LIB_EXPR, str(tmp_path / "child.npz"))


@pytest.mark.parametrize("name", CASES)
def test_search_routes(lib, L, model_path, name):
    KF.check_search_routes(F(lib, name, model_path), L, sdist, capi, want_both=name in ("B256", "B9000"))


def test_id_routes_and_edges(lib, model_path):
    """the ID route of every panel of every case with a dense reference, predicted and counted; the cases together put a panel
    on each side of each limit of the ID"""
    table = []
    for name in DENSE_CASES + ["A_gauss"]:
        table += KF.check_id_routes(F(lib, name, model_path), KM, lib)
    KF.check_edges(table, lib)


def test_generators_of_the_large_case(lib, model_path):
    KF.check_generators_large(F(lib, "B9000", model_path))


@pytest.mark.parametrize("name", B_CASES)
def test_doubling_leaves_nothing_behind(lib, model_path, name):
    KF.check_doubling_is_clean(F(lib, name, model_path), KM, lib)


@pytest.mark.parametrize("k", KF.KNN_DOUBLED)
def test_knn_at_doubled_counts(hk, k):
    KF.check_knn_doubled(hk, k, filter_min=600)


def test_colsets_at_256_neighbours(hk):
    KF.check_colsets_wide(hk)
