"""The kernel ridge regression fit at high ranks and after neighbour doubling, shared by the CPU emulator tests
(tests/test_kfit_emu.py) and the GPU tests (tests/test_kfit_gpu.py), as tests/gp_cases.py is.

Every fit is KernelRegression(..., keep_model=True) with --hss_leaf_size 128 --hss_clustering_algorithm cobble and the library's
own neighbour search, on uniform points of the unit cube (numpy default_rng(seed).random((n, d))), lambda = 3.11.

The cases (n, d, kernel, h, rel_tol, first neighbour count, seed) and what they reached when they were chosen (emulator | MI355X):
  A      (1500, 8, Laplace, 4.0, 1e-2, 64, 1)   one round, neighbours 64; largest rank 188 against 43 for the Gauss h = 1.3
         rel_tol 1e-2 fit of the same points (4.4 times; asked for: 2.5 times), inner nodes of up to 371 rows (asked for: more
         than 256): the 16 leaves (93 / 94 rows) end at full rank, the 8 panels above them (187 / 188 rows, ranks 177 .. 187) outgrow
         the rows the Gram ID holds and are redone by the Householder ID, the 6 panels of 346 .. 371 rows are beyond
         hssk_pchol_id_max_m(); no inner level fits the fused ULV step, the solve sweep declines.
  A_gauss (1500, 8, Gauss, 1.3, 1e-2, 64, 1)    the baseline of A and its counterpart: largest rank 43, all 30 panels in the Gram
         ID, three inner levels in the fused ULV step and one (the lowest: panels of 79 .. 84 rows) outside it, the single-launch
         solve sweep taken
  B128s  (600, 2, Laplace, 1.0, 3e-5, 64, 1)    two rounds, neighbours 128 < 150; largest rank 192, panels of up to 360 rows
  B128   (1000, 2, Laplace, 1.0, 3e-5, 64, 1)   two rounds, neighbours 128 < 250; largest rank 252, panels of up to 478 rows
         (rel_tol 1e-4 stops at 64 neighbours and 1e-5 goes on to 256: 3e-5 sits in the middle of the decade between them;
         GPU tier only, to keep the emulator tier short)
  B256   (1100, 2, Laplace, 1.0, 1e-5, 64, 1)   three rounds, neighbours 256 < 275 (also with seed 2); largest rank 348, panels of
         up to 685 rows: with HSSK_KNN_FILTER_MIN=600 the filtered search answers the rounds of 64 and 128 neighbours and the
         paged heap search (4 pages) the last one
  B9000  (9000, 2, Laplace, 1.0, 5e-6, 64, 2)   GPU tier only: three rounds, neighbours 256 < 2250; largest rank 1213, panels of
         up to 2261 rows; the default HSSK_KNN_FILTER_MIN (8192) gives the rounds of 64 and 128 neighbours to the filtered
         search (rel_tol 1e-5 stops at 128 neighbours, which the case also accepts; 1e-6 goes on to 1024)
The numbers are the same on the emulator and on the MI355X.  The regime conditions are asserted by check_regime; a case that
stops reaching them fails there.  The edges of DeviceHSS::id_panels are met on both sides by the cases of a tier together
(check_edges: panels of 68 .. 543 rows around hssk_pchol_id_max_m(), column sets of 154 .. 1026 ids around max(256, 2 m), ranks
below, at and above hssk_pchol_id_rank_cap(m)), those of factor_level and the sweeps between A and A_gauss
(expected_fit_routes).  The exact pairs m = limit, limit + 1 are not met: a point set cannot be tuned to a panel of exactly 256
skeleton rows.  Limits that have a query function are read from it at test time.  Those that have none are copied from the
sources -- 256 rows of the single-launch sweeps (SWEEP_MAX_ROWS), k <= 128, n >= 8192 and d <= 29 or d > 64 of the filtered
search (expected_filtered_rounds), the tolerance floor 1e-6 and max(256, 2 m) of the Gram ID (id_routes) -- as hss_cases does:
a change of one of them in the kernels needs the matching edit here.

What a case checks.  ||Hd - K||_F / ||K||_F measured for check 1, fit | oracle: A 7.817e-3 | 7.817e-3, A_gauss 6.907e-3 | 6.907e-3,
B128s 2.207e-4 | 2.207e-4, B128 1.969e-4 | 1.969e-4, B256 4.492e-5 | 4.492e-5 (equal to the digits shown: no tie came out
differently); leaf blocks at 0.36 of their entry bound.  B9000 has no dense form (1.3 GB in long double): checks 1 and 2 run
against the written generators applied by numpy (check_generators_large: backward error of the weights 6.4e-17, 24 sampled
rows at 6.3e-5 of their norm = 12.6 rel_tol, under the 100 rel_tol test_kernel_gpu.py allows sampled rows).
  1  the dense form of the kept model (gp_cases.dense_model) against K + lambda I in long double (kernel_cases.kernel_ref) in
     cluster order: the diagonal leaf blocks entry by entry under kernel_cases.kernel_entry_bound, the whole matrix in the
     Frobenius norm relative to ||K||_F under TWICE the same error of the numpy oracle (oracle.hss_oracle.HSSMatrix.from_kernel:
     same tree, exact neighbour lists of the final count, same tolerances) -- twice because the oracle takes another pivot
     order in ties.  Measured (fit | oracle): see DESIGN.md 8h.
  2  weights() against numpy.linalg.solve(Hd, y): ||w - w_ref|| <= 1e-12 cond_2(Hd) ||w_ref|| (gp_cases.EPS_F, the forward error
     the project accepts for the ULV solve; Hd is the compressed matrix, so this is rounding only)
  3  the same fit in a child process with STRUMPACK_AMD_ID_GRAM=0 STRUMPACK_AMD_ID_GRAM_GEN=0 STRUMPACK_AMD_KERNEL_HOST_SETS=1
     HSSK_KNN_FILTER=0: the same permutation, tree and final neighbour count; ranks one off on at most a twentieth of the nodes
     (the allowance of test_kernel_gpu.py's front-end comparison); no panel of the child in the Gram ID, and the column-set sizes
     summed over all panels and rounds, plain and weighted by the node, equal to this process's (SPX_id_route_counts)
  4  the launch counters around the fit against the routes predicted from the node table and the query functions
     (expected_fit_routes): hssk_ulv_node_launches, hssk_sweep_fused_launches / hssk_sweep_fallbacks; and, through the
     structured interface on the same points (SPX_d_struct_from_kernel: its context is reachable), the rounds, the final
     neighbour count, the node table of the fit and the number of rounds the filtered search answered (expected_filtered_rounds)
     and the row IDs (check_id_routes): per panel the route id_routes predicts from the node table, the numpy column sets and
     the library's limits, against the panels DeviceHSS::id_panels counted for the Gram ID, for its redo by the Householder ID
     and for the Householder ID at once in one round at the final neighbour count; the summed column-set sizes with them.
     hssk_sweep_chain_ok is only queried: a fit solves once from the host and builds no chain blocks (asserted: no chain launch);
     hssk_id_group_launches is printed, not predicted
  5  (B) the fit that doubled to k equals bit for bit a fresh fit started with --hss_approximate_neighbors k: node table,
     permutation, weights, logabsdet
  6  direct kernel checks at the sizes the doubled rounds produce: kernel_cases.case_knn at k = 128, 129, 192, 256 (n = 1100,
     d = 8) and hssk_colsets on leaves of 128 x 256 ids over 9000 points with a parent that unites two of them (check_colsets_wide)
"""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np

import gp_cases as GP
import hss_cases as HC
import kernel_cases as KC
from oracle import hss_oracle as O
from strumpack_amd import hssk as K

LD = np.longdouble
LAM = 3.11
LEAF = 128
KERNEL = {"gauss": ("rbf", "Gauss", 0), "laplace": ("Laplace", "Laplace", 1)}
# name: (n, d, kernel, h, rel_tol, seed, neighbour counts allowed at the end)
CASES = {
    "A": (1500, 8, "laplace", 4.0, 1e-2, 1, (64,)),
    "A_gauss": (1500, 8, "gauss", 1.3, 1e-2, 1, (64,)),
    "B128s": (600, 2, "laplace", 1.0, 3e-5, 1, (128, 256)),
    "B128": (1000, 2, "laplace", 1.0, 3e-5, 1, (128, 256)),
    "B256": (1100, 2, "laplace", 1.0, 1e-5, 1, (128, 256)),
    "B9000": (9000, 2, "laplace", 1.0, 5e-6, 2, (128, 256)),
}
SECOND_ROUTE = {"STRUMPACK_AMD_ID_GRAM": "0", "STRUMPACK_AMD_ID_GRAM_GEN": "0", "STRUMPACK_AMD_KERNEL_HOST_SETS": "1", "HSSK_KNN_FILTER": "0"}
SWEEP_MAX_ROWS = 256          # the single-launch sweeps take nodes of up to 256 rows (hss_cases.expected_routes has the same limit)
KNN_FILTER_MAX_K, KNN_FILTER_DEFAULT_MIN = 128, 8192      # include/hssk.h, hssk_knn
DENSE_MAX = 4096              # cases beyond it have no dense reference (B9000: 1.3 GB in long double)


def points(name):
    n, d, _, _, _, seed, _ = CASES[name]
    r = np.random.default_rng(seed)
    X = r.random((n, d))
    y = np.where(X[:, 0] + 0.1 * r.standard_normal(n) > 0.5, 1.0, -1.0)
    return X, y


def fit_args(name, ann=None):
    a = ["--hss_leaf_size", str(LEAF), "--hss_clustering_algorithm", "cobble", "--hss_rel_tol", repr(CASES[name][4])]
    return a + (["--hss_approximate_neighbors", str(ann)] if ann else [])


@contextlib.contextmanager
def environment(env):
    """os.environ with `env` on top (hssk_knn reads HSSK_KNN_FILTER_MIN at every call)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fit(KM, lib, name, env, ann=None):
    X, y = points(name)
    _, _, kern, h, _, _, _ = CASES[name]
    with environment(env):
        return KM.KernelRegression(lib, h=h, lam=LAM, kernel=KERNEL[kern][0], argv=fit_args(name, ann), keep_model=True).fit(X, y)


def id_route_counts(lib):
    """SPX_id_route_counts: panels given to the Gram ID, those of them redone by the Householder ID, panels given to the Householder
    ID at once, sum of the panels' sample rows (the sizes of the column sets), the same weighted by the node"""
    out = np.zeros(5, dtype=np.int64)
    lib.SPX_id_route_counts.argtypes, lib.SPX_id_route_counts.restype = [ctypes.c_void_p], None
    lib.SPX_id_route_counts(out.ctypes.data)
    return out


class Fitted:
    """one fit of a case with what the checks share: the node table, the counters around the fit, the dense form"""

    def __init__(self, KM, lib, name, env, path):
        self.name, self.env = name, dict(env)
        HC.sweep_counters(lib)
        lib.hssk_id_group_launches.restype = ctypes.c_longlong
        c0, g0, r0 = HC.sweep_counters(lib), lib.hssk_id_group_launches(), id_route_counts(lib)
        self.kr = fit(KM, lib, name, env)
        self.delta, self.group_launches = HC._delta(lib, c0), lib.hssk_id_group_launches() - g0
        self.id_counts = id_route_counts(lib) - r0
        self.T = self.kr.node_info()
        self.kids, self.height = GP.tree_of(self.T)
        self.info = self.kr.info()
        self.k = int(self.info["neighbors"])
        self.path = path
        self._dense = self._oracle = self._fresh = None

    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle_fit(self)
        return self._oracle

    def final_round(self, KM, lib):
        """(fit, its ID route counts) of ONE round at the final neighbour count: the fit itself where it did not double, else a
        fresh fit started there (the one check 5 compares with)"""
        if self.k == 64:
            return self.kr, self.id_counts
        if self._fresh is None:
            r0 = id_route_counts(lib)
            kr = fit(KM, lib, self.name, self.env, ann=self.k)
            self._fresh = (kr, id_route_counts(lib) - r0)
        return self._fresh

    def dense(self):
        if self._dense is None:
            self._dense = GP.dense_model(self.kr, self.path)
        return self._dense

    def inner(self):
        return [i for i in range(len(self.T)) if self.kids[i]]

    def rows(self, i):
        """rows of the ID panel of node i: its own (leaf), its children's ranks"""
        return int(self.T[i][1]) if not self.kids[i] else int(self.T[self.kids[i][0]][3] + self.T[self.kids[i][1]][3])


_FITS = {}


def fitted(KM, lib, name, env, path):
    key = (name, tuple(sorted(env.items())))
    if key not in _FITS:
        _FITS[key] = Fitted(KM, lib, name, env, path)
    return _FITS[key]


def release():
    for f in _FITS.values():
        f.kr.destroy()
        if f._fresh is not None:
            f._fresh[0].destroy()
    _FITS.clear()


# ---- the regime ---------------------------------------------------------------------------------------------------------------------
def check_regime(F, base=None):
    """the conditions the case is there for (module docstring); base: the Gauss fit of the same points (case A)"""
    n = CASES[F.name][0]
    T = F.T
    assert F.info["compressed"] == 1
    assert F.k in CASES[F.name][6], (F.name, F.k)
    m_inner = [F.rows(i) for i in F.inner()]
    print("regime %s: neighbours %d, largest rank %d, largest inner panel %d rows, levels %d" % (F.name, F.k, T[:, 3].max(), max(m_inner), F.info["levels"]))
    if F.name == "A":
        assert T[:, 3].max() >= 2.5 * base.T[:, 3].max(), (T[:, 3].max(), base.T[:, 3].max())
        assert max(m_inner) > SWEEP_MAX_ROWS and max(m_inner) > F.kr.L.hssk_pchol_id_max_m(), m_inner
    if F.name.startswith("B"):
        assert F.k in (128, 256) and 4 * F.k < n, (F.k, n)


def id_routes(F, lib, sizes):
    """per node below the root the route of its ID as DeviceHSS::id_panels chooses it, from the panel's rows m, the size d of its
    column set (`sizes`: the numpy column sets of the exact neighbour lists) and the library's own limits:
    'gram' (m <= hssk_pchol_id_max_m(), d > max(256, 2 m), rel_tol / level >= 1e-6, rank within hssk_pchol_id_rank_cap(m)),
    'gram_overflow' (the same, but the rank needs more rows than the Gram kernel holds: the Householder ID follows), 'qr'"""
    rel = CASES[F.name][4]
    lvl = {0: 0}
    for i in F.inner():
        for c in F.kids[i]:
            lvl[c] = lvl[i] + 1
    out = {}
    for i in range(1, len(F.T)):
        m, d, r = F.rows(i), int(sizes[i]), int(F.T[i][3])
        if m <= 0 or m > lib.hssk_pchol_id_max_m() or d <= max(256, 2 * m) or rel / lvl[i] < 1e-6:
            out[i] = "qr"
        else:
            cap = max(1, min(m, lib.hssk_pchol_id_rank_cap(m)))
            # (the kernel gives up when it has filled its cap rows without meeting the tolerance: a rank of exactly cap may be either)
            out[i] = "gram" if r < cap else ("gram_overflow" if r > cap else "gram_edge")
    return out


def expected_fit_routes(F, lib):
    """(levels of the factorization that take hssk_ulv_node_vbatched, the solve's single-launch sweep is taken) -- DeviceHSS::
    factor_level fuses a level of inner nodes when every node of it fits (hssk_ulv_node_fits) and eliminates; the sweep declines a
    tree with a node of more than 256 rows"""
    T, levels = F.T, {}
    for i in F.inner():
        a, b = F.kids[i]
        mu = int(T[a][3] + T[b][3])
        root = i == 0
        ok = mu > 0 and (root or (int(T[i][2]) == mu and mu > int(T[i][3])))
        ok = ok and bool(lib.hssk_ulv_node_fits(mu, 0 if root else int(T[i][3]), 0 if root else int(T[i][4]), int(T[a][3]), int(T[b][3]), int(T[a][4]), int(T[b][4])))
        levels.setdefault(F.height[i], []).append(ok)
    fused = sum(1 for v in levels.values() if all(v))
    mixed = any(all(v) for v in levels.values()) and any(not all(v) for v in levels.values())
    sweep = all(F.rows(i) <= SWEEP_MAX_ROWS for i in range(len(T)))
    return fused, sweep, mixed


def check_counters(F, lib):
    """check 4, the counters around the fit itself"""
    fused, sweep, mixed = expected_fit_routes(F, lib)
    d = F.delta
    print("routes %s: fused ULV levels expected %d, counters %s, group ID launches %d" % (F.name, fused, d, F.group_launches))
    if not HC.env_flag("NO_ULV_NODE"):
        assert d["ulv_node_launches"] == fused, (F.name, d, fused)
    if not HC.env_flag("NO_FUSED_SOLVE"):
        assert (d["sweep_fused_launches"] > 0) == sweep and (d["sweep_fallbacks"] > 0) == (not sweep), (F.name, d, sweep)
    inner, ok = 0, 0
    for i in F.inner()[1:]:
        a, b = F.kids[i]
        m = F.rows(i)
        if m > int(F.T[i][3]):
            inner += 1
            ok += int(lib.hssk_sweep_chain_ok(m, int(F.T[i][3]), int(F.T[a][4] + F.T[b][4]), int(F.T[i][4])))
    print("routes %s: %d of %d inner nodes below the root have a shape hssk_sweep_chain_ok takes" % (F.name, ok, inner))
    # (chain blocks are built before the second single-vector solve on a device buffer only -- DeviceHSS::chain_blocks -- and a fit
    #  solves once, from the host: the query above says what such a solve would find, the counter that none ran)
    assert d["sweep_chain_launches"] == 0, d
    if F.name != "A_gauss":
        assert fused == 0 and not sweep and ok < inner, (fused, sweep, ok, inner)       # every route of the low-rank fit is left
    if F.name == "A_gauss":
        assert mixed and sweep, (fused, sweep)          # a level inside the fused step, another outside it
    return fused, sweep


def expected_filtered_rounds(n, d, k0, k_final, env):
    """the rounds of neighbour counts k0, 2 k0, .. k_final that hssk_knn gives to the filtered search (include/hssk.h)"""
    fmin = int(env.get("HSSK_KNN_FILTER_MIN", KNN_FILTER_DEFAULT_MIN))
    ks, k = [], k0
    while k <= k_final:
        ks.append(k)
        k *= 2
    on = env.get("HSSK_KNN_FILTER", "1") != "0"
    return len(ks), sum(1 for k in ks if on and n >= fmin and k <= KNN_FILTER_MAX_K and (d <= 29 or d > 64) and n > 4 * k)


def check_search_routes(F, L, sdist, capi, want_both=False):
    """check 4, the neighbour search: the same points through SPX_d_struct_from_kernel, whose context is reachable
    (SPX_d_struct_hssk_ctx; new with the matrix, so its filtered count is that of this compression alone)"""
    n, d, kern, h, rel, _, _ = CASES[F.name]
    X, _ = points(F.name)
    o = capi.StructuredMatrix.options(L, rel_tol=rel, abs_tol=1e-8, leaf_size=LEAF)
    with environment(F.env):
        H, Xp, perm = sdist.from_kernel(L, X, o, kernel=KERNEL[kern][1], h=h, lam=LAM, clustering="cobble", neighbors=64)
    try:
        st = H.stats()
        L.hssk_knn_filtered_count.argtypes, L.hssk_knn_filtered_count.restype = [ctypes.c_void_p], ctypes.c_longlong
        took = L.hssk_knn_filtered_count(L.SPX_d_struct_hssk_ctx(H.h))
        rounds, filt = expected_filtered_rounds(n, d, 64, F.k, F.env)
        print("search %s: rounds %d, final neighbours %d, rounds of the filtered search %d (expected %d of %d)" % (F.name, st["rounds"], st["d_final"], took, filt, rounds))
        assert int(st["d_final"]) == F.k and int(st["rounds"]) == rounds, (st["d_final"], st["rounds"], F.k, rounds)
        assert took == filt, (took, filt)
        if want_both:
            assert 0 < filt < rounds, "the case must take both searches"
        assert np.array_equal(perm, F.kr.permutation()) and np.array_equal(H.node_info(), F.T), "the structured interface compressed another matrix"
    finally:
        H.destroy()


# ---- 1, 2: the dense form and the solve ---------------------------------------------------------------------------------------------
def exact_neighbours(Xp, k):
    n = len(Xp)
    D2 = np.zeros((n, n))
    for j in range(Xp.shape[1]):
        D2 += (Xp[:, j][:, None] - Xp[:, j][None, :]) ** 2
    np.fill_diagonal(D2, np.inf)
    return np.argpartition(D2, k - 1, axis=1)[:, :k].astype(np.int64)


def oracle_fit(F):
    """the numpy restatement of the compression on the fit's own tree, with exact neighbour lists of the final count"""
    _, _, kern, h, rel, _, _ = CASES[F.name]
    Xp = F.kr.model_points()
    H = O.HSSMatrix.from_kernel(Xp, O.kernel_function(KERNEL[kern][2], h, 1), LAM, F.T[:, 1], F.T[:, 5], exact_neighbours(Xp, F.k),
                                O.Options(rel_tol=rel, abs_tol=1e-8, leaf_size=LEAF))
    assert H.is_compressed(), "the oracle did not compress with the fit's neighbour count"
    return H


def check_dense(F, lib):
    """checks 1 and 2; returns (error of the fit, error of the oracle), both ||. - K||_F / ||K||_F"""
    _, d, kern, h, _, _, _ = CASES[F.name]
    ktype = KERNEL[kern][2]
    Hd, sv, R = F.dense()
    Xp = F.kr.model_points()
    n = len(Xp)
    idx = np.arange(n)
    Kx, a, A = KC.kernel_ref(Xp, idx, idx, ktype, h, LAM)
    b = KC.kernel_entry_bound(a, A, ktype, d, LAM)
    worst = 0.0
    for i in range(len(F.T)):
        if F.T[i][5]:
            lo, m = int(F.T[i][0]), int(F.T[i][1])
            s = slice(lo, lo + m)
            err = np.abs(Hd[s, s].astype(LD) - Kx[s, s])
            worst = max(worst, float((err / b[s, s]).max()))
            assert np.all(err <= b[s, s]), (F.name, i, worst)
    nK = float(np.sqrt((Kx * Kx).sum()))
    e_fit = float(np.sqrt(((Hd.astype(LD) - Kx) ** 2).sum())) / nK
    Ho = F.oracle()
    e_or = float(np.sqrt(((Ho.dense().astype(LD) - Kx) ** 2).sum())) / nK
    ro = np.array([nd.rU for nd in Ho.nodes])
    print("dense %s n=%d: leaf blocks largest error / bound %.3f; ||Hd - K||_F / ||K||_F fit %.3e oracle %.3e; largest rank fit %d oracle %d"
          % (F.name, n, worst, e_fit, e_or, F.T[:, 3].max(), ro.max()))
    assert e_fit <= 2.0 * e_or, (F.name, e_fit, e_or)
    # 2: the solve
    y, w = F.kr.model_labels(), F.kr.weights()
    wr = np.linalg.solve(Hd, y)
    cond = sv[0] / sv[-1]
    fe = np.linalg.norm(w - wr) / np.linalg.norm(wr)
    print("solve %s: cond %.3g, ||w - w_ref|| / ||w_ref|| %.3g (bound %.3g)" % (F.name, cond, fe, GP.EPS_F * cond))
    assert fe <= GP.EPS_F * cond, (F.name, fe, cond)
    return e_fit, e_or


def check_id_routes(F, KM, lib):
    """check 4, the row IDs: the routes id_routes predicts for one round at the final neighbour count -- from the node table, the
    numpy column sets of the exact neighbour lists and the library's limits -- against what DeviceHSS::id_panels counted
    (SPX_id_route_counts) in such a round; the sum of the column-set sizes with them.  Returns the per-node table for check_edges."""
    sizes = {nd.idx: len(nd.cols) for nd in F.oracle().nodes if nd.lvl > 0}
    kr, got = F.final_round(KM, lib)
    assert np.array_equal(kr.node_info(), F.T)
    routes = id_routes(F, lib, sizes)
    count = {k: sum(1 for v in routes.values() if v == k) for k in ("gram", "gram_edge", "gram_overflow", "qr")}
    rows = sum(max(sizes[i], 1) for i in routes)          # (an empty column set is a 1 x m panel of zeros)
    print("ID routes %s: predicted %s, column-set sizes %d; counted Gram %d, redone %d, Householder %d, sizes %d"
          % (F.name, count, rows, got[0], got[1], got[2], got[3]))
    assert got[0] == count["gram"] + count["gram_edge"] + count["gram_overflow"], (got, count)
    assert got[2] == count["qr"], (got, count)
    # (a panel whose rank is exactly the rows the Gram kernel holds may or may not have met the tolerance there)
    assert count["gram_overflow"] <= got[1] <= count["gram_overflow"] + count["gram_edge"], (got, count)
    assert got[3] == rows, (got[3], rows)
    table = []
    for i, route in routes.items():
        m = F.rows(i)
        table.append((F.name, i, m, int(sizes[i]), int(F.T[i][3]), max(1, min(m, lib.hssk_pchol_id_rank_cap(m))), route))
    return table


def check_edges(table, lib):
    """the cases of a tier together: a panel on each side of each limit of DeviceHSS::id_panels (section C of the cases)"""
    mx = lib.hssk_pchol_id_max_m()
    small = [t for t in table if t[2] <= mx]
    print("edges: panels of %d .. %d rows (limit %d); of those within it, column sets of %d .. %d ids; Gram panels with rank - cap in %s"
          % (min(t[2] for t in table), max(t[2] for t in table), mx, min(t[3] for t in small), max(t[3] for t in small),
             sorted(set(t[4] - t[5] for t in table if t[6] != "qr"))[:: 8]))
    assert small and len(small) < len(table), "no panel on one side of hssk_pchol_id_max_m()"
    assert any(t[3] > max(256, 2 * t[2]) for t in small) and any(t[3] <= max(256, 2 * t[2]) for t in small), "d = max(256, 2 m)"
    gram = [t for t in table if t[6] != "qr"]
    assert any(t[4] < t[5] for t in gram) and any(t[4] > t[5] for t in gram) and any(t[4] == t[5] for t in gram), "rank against hssk_pchol_id_rank_cap(m)"


# ---- 3: the second route ------------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(here)r); sys.path.insert(0, %(root)r)
import kfit_cases as KF
from strumpack_amd import kernel as KM
%(lib_expr)s
lib = KM.load(path)
kr = KF.fit(KM, lib, %(name)r, {}, %(ann)r)
np.savez(sys.argv[1], perm=kr.permutation(), nodes=kr.node_info(), k=kr.info()["neighbors"], w=kr.weights(), ids=KF.id_route_counts(lib))
kr.destroy()
"""


def child_fit(lib_expr, name, env, out, ann=None, timeout=900):
    """the fit of a case in a fresh process under `env`"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = CHILD % dict(here=here, root=os.path.dirname(here), lib_expr=lib_expr, name=name, ann=ann)
    r = subprocess.run([sys.executable, "-c", code, out], env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return np.load(out)


def check_second_route(F, lib_expr, out):
    Z = child_fit(lib_expr, F.name, dict(F.env, **SECOND_ROUTE), out)
    assert np.array_equal(Z["perm"], F.kr.permutation()), "permutation"
    assert int(Z["k"]) == F.k, (int(Z["k"]), F.k)
    assert np.array_equal(Z["nodes"][:, [0, 1, 5]], F.T[:, [0, 1, 5]]), "tree"
    dr = np.abs(Z["nodes"][:, 3:5].astype(int) - F.T[:, 3:5].astype(int))
    w = F.kr.weights()
    print("second route %s: ranks differ on %d of %d nodes (largest difference %d), ||w - w'|| / ||w|| %.3g"
          % (F.name, int((dr[:, 0] > 0).sum()), len(dr), int(dr.max()), np.linalg.norm(Z["w"] - w) / np.linalg.norm(w)))
    assert dr.max() <= 1 and (dr > 0).mean() <= 0.05, (int(dr.max()), float((dr > 0).mean()))
    # the routes did change, and the column sets did not: no panel in the Gram ID, the same sizes node by node over all rounds
    ids = Z["ids"]
    print("second route %s: ID route counts %s, here %s" % (F.name, ids.tolist(), F.id_counts.tolist()))
    assert ids[0] == 0 and ids[1] == 0 and ids[2] == F.id_counts[0] + F.id_counts[2], (ids, F.id_counts)
    assert ids[3] == F.id_counts[3] and ids[4] == F.id_counts[4], "column-set sizes"
    if F.T[0][1] > DENSE_MAX:
        # no dense form at this size: the residual on sampled rows of the exact matrix against the same residual of the second
        # route's weights (the same permutation, hence the same rows and labels), twice of it as in check 1
        e, e2 = sampled_residual(F, w), sampled_residual(F, Z["w"])
        print("sampled rows %s: residual %.3e, second route %.3e" % (F.name, e, e2))
        assert e <= 2.0 * e2, (e, e2)


# ---- 5: doubling leaves nothing behind ----------------------------------------------------------------------------------------------
def check_doubling_is_clean(F, KM, lib):
    assert F.k > 64, "the case did not double"
    fresh = F.final_round(KM, lib)[0]
    assert fresh is not F.kr and fresh.info()["neighbors"] == F.k
    assert np.array_equal(fresh.node_info(), F.T), "node table"
    assert np.array_equal(fresh.permutation(), F.kr.permutation()), "permutation"
    assert np.array_equal(fresh.weights(), F.kr.weights()), "weights"
    assert fresh.logabsdet() == F.kr.logabsdet(), (fresh.logabsdet(), F.kr.logabsdet())


# ---- the large case: no dense form ----------------------------------------------------------------------------------------------------
def sampled_residual(F, w, rows=24, seed=3):
    """||(K + lambda I)_I w - y_I|| / ||y_I|| on sampled rows I of the exact matrix (long double): the compression error of the fit
    behind w, seen through its solve"""
    _, d, kern, h, rel, _, _ = CASES[F.name]
    Xp, y = F.kr.model_points(), F.kr.model_labels()
    n = len(Xp)
    I = np.random.default_rng(seed).integers(0, n, rows)
    KI = KC.kernel_ref(Xp, I, np.arange(n), KERNEL[kern][2], h, LAM)[0]
    res = np.asarray(KI @ w.astype(LD), dtype=np.float64) - y[I]
    return float(np.linalg.norm(res) / np.linalg.norm(y[I]))


def check_generators_large(F, rows=24, seed=3):
    """checks 1 and 2 where no dense form fits (B9000), against the generators the kept model writes, applied by numpy
    (hss_generators), as hss_cases.check_against_generators does beyond 4096 rows:
    2  backward error of weights() in the compressed matrix, ||H w - y|| / (||H||_2 ||w|| + ||y||) <= hss_cases.GEN_TOL;
    1  sampled rows I of the generator form against the same rows of K + lambda I in long double: the entries inside the row's
       own leaf under kernel_cases.kernel_entry_bound, the rows in the Frobenius norm under 100 rel_tol, the allowance
       test_kernel_gpu.py gives sampled rows of a compressed kernel matrix (the dense cases and their oracle sit at 0.8 - 7.4
       rel_tol with half as many levels)"""
    import hss_generators as G
    _, d, kern, h, rel, _, _ = CASES[F.name]
    ktype = KERNEL[kern][2]
    F.kr.write_model(F.path)
    R = G.read(F.path)
    os.remove(F.path)
    Xp, y, w = F.kr.model_points(), F.kr.model_labels(), F.kr.weights()
    n = len(Xp)
    nH = R.norm2(iters=15)
    be = np.linalg.norm(R.apply(w[:, None])[:, 0] - y) / (nH * np.linalg.norm(w) + np.linalg.norm(y))
    I = np.random.default_rng(seed).integers(0, n, rows)
    E = np.zeros((n, rows))
    E[I, np.arange(rows)] = 1.0
    HI = R.apply(E, "T").T
    KI, a, A = KC.kernel_ref(Xp, I, np.arange(n), ktype, h, LAM)
    b = KC.kernel_entry_bound(a, A, ktype, d, LAM)
    worst = 0.0
    leaves = [(int(t[0]), int(t[0] + t[1])) for t in F.T if t[5]]
    for q, i in enumerate(I):
        lo, hi = next(lh for lh in leaves if lh[0] <= i < lh[1])
        err = np.abs(HI[q, lo:hi].astype(LD) - KI[q, lo:hi])
        worst = max(worst, float((err / b[q, lo:hi]).max()))
    e = float(np.sqrt(((HI.astype(LD) - KI) ** 2).sum()) / np.sqrt((KI * KI).sum()))
    print("generators %s: backward error of the weights %.3g (bound %.3g); sampled rows: leaf entries largest error / bound %.3f, "
          "||H_I - K_I||_F / ||K_I||_F %.3e (bound %.3e)" % (F.name, be, HC.GEN_TOL, worst, e, 1e2 * rel))
    assert be <= HC.GEN_TOL, be
    assert worst <= 1.0, worst
    assert e <= 1e2 * rel, e


# ---- 6: the kernels at the sizes of the doubled rounds --------------------------------------------------------------------------------
KNN_DOUBLED = (128, 129, 192, 256)      # both sides of the filtered search's limit; 2, 3, 3 and 4 pages of the heap search


def check_knn_doubled(hk, k, filter_min=None):
    """kernel_cases.case_knn at n = 1100, d = 8; filter_min lowers the threshold of the filtered search below n (as
    kernel_cases.case_knn_filter_edges does): the context's counter says which search answered the two calls"""
    n, d = 1100, 8
    env = {} if filter_min is None else {"HSSK_KNN_FILTER_MIN": str(filter_min)}
    c0 = hk.lib.hssk_knn_filtered_count(hk.ctx)
    with environment(env):
        KC.case_knn(hk, n=n, d=d, k=k, seed=1100 + k)
    took = hk.lib.hssk_knn_filtered_count(hk.ctx) - c0
    _, want = expected_filtered_rounds(n, d, k, k, env)
    assert took == 2 * want, (k, took, want)


def check_colsets_wide(hk, universe=9000, m=128, k=256, seed=83):
    """hssk_colsets at what a round of 256 neighbours gives it: two leaves of 128 points with 256 neighbour ids each (32768 ids
    per leaf, -1 among them), then their parent, which reads the children's counts on the device (n0_dev / n1_dev) with the
    launch bounds as n0 / n1, as DeviceHSS::compress_kernel launches its levels back to back"""
    r = np.random.default_rng(seed)
    lo0, lo1 = 4000, 4000 + m
    leaves = []
    for lo in (lo0, lo1):
        ids = r.integers(-1, universe, size=m * k).astype(np.int32)
        ids[:: 7] = r.integers(lo - 300, lo + 300, size=len(ids[:: 7]))      # many near the leaf, some inside it
        leaves.append((ids, lo, lo + m))
    dev, descs = [], []
    for ids, lo, hi in leaves:
        src, out = hk.array(ids), hk.array(np.full(len(ids) + 1, -7, dtype=np.int32))
        cnt = hk.array(np.full(1, -3, dtype=np.int32))
        dev.append((src, out, cnt))
        descs.append(K.ColsetDesc(src.ptr, None, len(ids), 0, lo, hi, out.ptr, cnt.ptr, None, None))
    arr = (K.ColsetDesc * 2)(*descs)
    hk.check(hk.lib.hssk_colsets(hk.ctx, arr, 2, universe))
    refs = []
    for (ids, lo, hi) in leaves:
        refs.append(np.unique(ids[(ids >= 0) & ((ids < lo) | (ids >= hi))]))
    bound = [min(m * k, universe - m)] * 2
    pout = hk.array(np.full(bound[0] + bound[1] + 1, -7, dtype=np.int32))
    pcnt = hk.array(np.full(1, -3, dtype=np.int32))
    parent = (K.ColsetDesc * 1)(K.ColsetDesc(dev[0][1].ptr, dev[1][1].ptr, bound[0], bound[1], lo0, lo1 + m, pout.ptr, pcnt.ptr, dev[0][2].ptr, dev[1][2].ptr))
    hk.check(hk.lib.hssk_colsets(hk.ctx, parent, 1, universe))
    hk.sync()
    for (src, out, cnt), ref in zip(dev, refs):
        c, got = int(cnt.get()[0]), out.get()
        assert c == len(ref) and np.array_equal(got[:c], ref) and np.all(got[c:] == -7), (c, len(ref))
    allv = np.concatenate(refs)
    pref = np.unique(allv[(allv < lo0) | (allv >= lo1 + m)])
    c, got = int(pcnt.get()[0]), pout.get()
    assert c == len(pref) and np.array_equal(got[:c], pref) and np.all(got[c:] == -7), (c, len(pref))
    assert len(refs[0]) > 4000 and len(pref) > len(refs[0]), "the sets are too small to prove anything"
    for t in dev:
        for v in t:
            v.free()
    pout.free()
    pcnt.free()
