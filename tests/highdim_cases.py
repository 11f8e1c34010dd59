"""Checks of kernel ridge regression on points of more than 64 coordinates, shared by the GPU tests (product library) and the CPU
tests (the same sources on the fiber emulator): the neighbour search, the FP64 prediction sum and the FP32 prediction sum beyond
R^64 -- where the coordinates of a point pass through the LDS in chunks instead of sitting in registers -- and the C interface end
to end on data of 100 and 784 coordinates.  The checkers, references and bounds are those of kernel_cases.py / kpredict_cases.py.

Chunk sizes the shapes below are chosen around: 32 coordinates per pass in the neighbour search and the FP64 sum (96 | 97 and
128 | 129 are chunk edges), 64 in the FP32 sum (128 | 129); 32 candidates per tile of the search, 32 (Gauss, Laplace) or 8 (ANOVA)
training points per tile of the FP64 sum, 32 (Gauss, Laplace) or 16 (ANOVA) per wave and sweep in the FP32 sum; 64 candidates per
tile and 16 operand rows per chunk in the filtered search."""
import contextlib
import os

import numpy as np

import kernel_cases as KC
import kpredict_cases as PC

# ---- neighbour search, general form: (n, d, k, lattice) ---------------------------------------------------------------------
# d = 65: the first dimension beyond the register form; 96 | 97 and 128 | 129: chunk edges; 200: a ragged last chunk;
# (300, 96, 70): two pages; (40, 65, 64): n - 1 < k, -1 padding; lattices: integer coordinates, ties ordered by index
KNN_GENERAL = ((150, 65, 10, False), (150, 96, 10, False), (150, 97, 10, False), (150, 128, 10, False), (150, 129, 10, False),
               (150, 200, 10, False), (300, 96, 70, False), (40, 65, 64, False), (150, 65, 10, True), (150, 130, 10, True))
# ---- neighbour search, filtered form (HSSK_KNN_FILTER_MIN = 600): (n, d, k, lattice, filtered) ------------------------------------
# The K loop takes the d + 2 rows of the augmented operand in chunks of 16: d = 65 (the first), 78 | 79 and 94 | 95 (d + 2 on
# either side of a chunk edge), 257 (beyond the 256 threads of the d <= 29 form's mean kernel), 784; k = 128 is the filter's last,
# k = 129 and n <= 4 k fall to the general form; a lattice (ties by index through the exact keys of the compaction)
KNN_FILTERED = tuple((700, d, 8, False, True) for d in (65, 78, 79, 94, 95, 257, 784)) + (
    (700, 65, 128, False, True), (700, 65, 129, False, False), (640, 65, 160, False, False), (700, 65, 8, True, True))


@contextlib.contextmanager
def filter_min(value):
    """HSSK_KNN_FILTER_MIN (read by hssk_knn at every call) set for the block, and the caller's setting put back after it"""
    before = os.environ.get("HSSK_KNN_FILTER_MIN")
    os.environ["HSSK_KNN_FILTER_MIN"] = str(value)
    try:
        yield
    finally:
        if before is None:
            os.environ.pop("HSSK_KNN_FILTER_MIN")
        else:
            os.environ["HSSK_KNN_FILTER_MIN"] = before


def case_knn_wide(hk, n, d, k, lattice):
    c0 = hk.lib.hssk_knn_filtered_count(hk.ctx)
    KC.case_knn(hk, n=n, d=d, k=k, seed=900 + d + k, lattice=lattice)
    assert hk.lib.hssk_knn_filtered_count(hk.ctx) == c0, "a small point set took the filtered search"


def case_knn_wide_filtered(hk, n, d, k, lattice, filtered):
    """kernel_cases.case_knn with the filter's threshold lowered the way case_knn_filter_edges lowers it; the context's counter
    shows which form answered the two calls (a silent fall to the general form would pass the result check)"""
    c0 = hk.lib.hssk_knn_filtered_count(hk.ctx)
    with filter_min(600):
        KC.case_knn(hk, n=n, d=d, k=k, seed=700 + d + k, lattice=lattice)
    took = hk.lib.hssk_knn_filtered_count(hk.ctx) - c0
    assert took == (2 if filtered else 0), "(n, d, k) = %s: %d of 2 calls took the filtered search" % ((n, d, k), took)


def case_knn_filtered_far_from_the_mean(hk, n=700, d=65, k=8):
    """Two clusters at +-1000 in every coordinate: every point is far from the mean, so the FP32 norm expansion
    |c|^2 + |q|^2 - 2 c.q of the filter is off by far more than the distances inside a cluster (u (|c|^2 + |q|^2) ~ 10 against
    squared distances ~ 130) and only the slack term of the pass threshold, 2.02 (K + 6) 2^-23 (|q|^2 + max |c|^2), keeps the true
    neighbours on the lists.  The check is kernel_cases.case_knn's: exactly a set of k nearest by the float keys."""
    r = KC.rng(31)
    X = r.standard_normal((n, d)) + np.where(r.random(n) < 0.5, 1000.0, -1000.0)[:, None]
    dX = hk.array(X.T)
    out = hk.empty((k, n), dtype=np.int32)
    c0 = hk.lib.hssk_knn_filtered_count(hk.ctx)
    with filter_min(600):
        hk.check(hk.lib.hssk_knn(hk.ctx, dX.ptr, d, n, k, 0, n // 3, out.ptr))
        hk.check(hk.lib.hssk_knn(hk.ctx, dX.ptr, d, n, k, n // 3, n, out.ptr))
        hk.sync()
    assert hk.lib.hssk_knn_filtered_count(hk.ctx) - c0 == 2
    got = out.get().T
    D2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1).astype(np.float32)
    np.fill_diagonal(D2, np.inf)
    for i in range(n):
        mine = got[i]
        assert (mine >= 0).all() and len(set(mine.tolist())) == k and i not in mine, i
        assert (D2[i][mine] <= np.sort(D2[i])[k - 1]).all(), "query %d: not a set of %d nearest" % (i, k)


# ---- FP64 prediction: (n, m, d) ---------------------------------------------------------------------------------------------
# the shapes of kernel_cases.PREDICT_SHAPES moved beyond R^64 (n and m on both sides of a workgroup's 64 test points and of the
# training tiles), the chunk edges 96 | 97 and 128 | 129, and R^784 with a ragged last tile of either kind
PREDICT_WIDE_SHAPES = ((1, 1, 65), (63, 64, 65), (64, 65, 129), (65, 1, 200), (130, 70, 784), (33, 10, 96), (33, 10, 97), (9, 3, 128))


def case_kernel_predict_wide(hk, n, m, d):
    return KC.case_kernel_predict(hk, n=n, m=m, d=d, seed=300 + d, kinds=((0, 1), (1, 1), (2, min(8, d))), widths=KC.kernel_widths(d))


# ---- FP32 prediction (hssk_kernel_predict_f32_wide) --------------------------------------------------------------------------
F32_WIDE_DIMS = (65, 96, 128, 129, 200, 784)


def f32_kinds(d):
    """(kernel type, ANOVA degree, width, tag): the widths of kernel_cases.kernel_widths, and a Gauss width that puts the exponents
    of a standard normal cloud near 6 -- a kernel that discriminates, where the error bound's (d + 4) a term is at its largest"""
    hg, hl, ha = KC.kernel_widths(d)
    return ((0, 1, hg, "gauss"), (0, 1, 0.4 * np.sqrt(d), "gauss narrow"), (1, 1, hl, "laplace"), (2, 1, ha, "anova p=1"),
            (2, 2, ha, "anova p=2"), (2, 8, ha, "anova p=8"))


def case_f32_wide(hk, d, n=257, m=70, kinds=None):
    """the checker of kpredict_cases (bound of DESIGN.md 8b, two runs bit for bit, statistics) on every kernel; every tile must
    have gone the difference form"""
    X, T, w = PC.points(100 + d, n, m, d)
    worst = 0.0
    for (kt, p, h, tag) in (kinds or f32_kinds(d)):
        frac, st = PC.check_predict(hk, X, T, w, kt, float(h), p, tag="%s d=%d" % (tag, d), routes="diff")
        worst = max(worst, frac)
    return worst


def case_f32_wide_sentinel(hk, d=65, n=130, m=70):
    """the floats behind the m outputs stay as they were, whatever the padding of the last test tile"""
    X, T, w = PC.points(3, n, m, d)
    dX, dT, dw = hk.array(X.ravel()), hk.array(T.ravel()), hk.array(w)
    for kt, p in ((0, 1), (1, 1), (2, 3)):
        dp = hk.array(np.full((m + 5,), KC.SENTINEL, dtype=np.float32))
        hk.check(hk.lib.hssk_kernel_predict_f32_wide(hk.ctx, dX.ptr, n, d, kt, p, 9.0, dw.ptr, dT.ptr, m, dp.ptr, None))
        hk.sync()
        got = dp.get()
        assert np.all(got[m:] == np.float32(KC.SENTINEL)), "hssk_kernel_predict_f32_wide wrote behind its m predictions"
        assert np.all(got[:m] != np.float32(KC.SENTINEL))
        dp.free()
    for a in (dX, dT, dw):
        a.free()


def case_f32_wide_errors(hk):
    """kpredict_cases.case_errors for the wide entry: it takes d >= 65 and refuses what hssk_kernel_predict_f32 takes"""
    d = 65
    X, T, w = PC.points(1, 64, 10, d)
    dX, dT, dw, dp = hk.array(X.ravel()), hk.array(T.ravel()), hk.array(w), hk.empty((10,), np.float32)
    f = hk.lib.hssk_kernel_predict_f32_wide

    def call(X=dX.ptr, n=64, d=d, kt=0, p=1, h=1.0, w=dw.ptr, T=dT.ptr, m=10, out=dp.ptr):
        return f(hk.ctx, X, n, d, kt, p, h, w, T, m, out, None)
    assert call() == 0
    for kw, word in ((dict(d=64), "dimension"), (dict(d=8), "dimension"), (dict(d=0), "dimension"), (dict(d=-3), "dimension"),
                     (dict(kt=3), "type"), (dict(kt=2, p=9), "degree"), (dict(kt=2, p=0), "degree"), (dict(X=None), "null"),
                     (dict(w=None), "null"), (dict(T=None), "null"), (dict(out=None), "null"), (dict(n=-1), "range"),
                     (dict(m=-1), "range"), (dict(n=1 << 40), "range"), (dict(h=0.0), "width")):
        assert call(**kw) != 0, kw
        assert word in hk.error(), (kw, hk.error())
    assert call(m=0, T=None, out=None) == 0
    st = np.zeros(6, dtype=np.int64)
    assert f(hk.ctx, dX.ptr, 0, d, 0, 1, 1.0, dw.ptr, dT.ptr, 10, dp.ptr, st.ctypes.data) == 0      # no training points: zeros
    hk.sync()
    assert np.array_equal(dp.get(), np.zeros(10, dtype=np.float32)) and not st.any()
    # the entries on either side of d = 64 | 65 refuse each other's dimension
    g = hk.lib.hssk_kernel_predict_f32
    assert g(hk.ctx, dX.ptr, 64, 65, 0, 1, 1.0, dw.ptr, dT.ptr, 10, dp.ptr, None) != 0 and "dimension" in hk.error()
    hk.sync()
    for a in (dX, dT, dw, dp):
        a.free()


# ---- the C interface end to end ---------------------------------------------------------------------------------------------
def clustered_points(seed, n, m, d, clusters=4, latent=3):
    """n training and m test points in R^d that a kernel matrix compresses on: a few Gaussian clusters whose spread lives in a
    `latent`-dimensional subspace, embedded by a random rotation (plus a little isotropic noise); squared distances are of order
    d, so a width h = sqrt(d) gives exponents of order one.  Labels +-1 by cluster."""
    r = np.random.default_rng(seed)
    Q = np.linalg.qr(r.standard_normal((d, d)))[0][:, :latent]
    centres = r.standard_normal((clusters, d))
    lab = r.integers(0, clusters, n + m)
    Z = centres[lab] + (r.standard_normal((n + m, latent)) * np.sqrt(d / latent)) @ Q.T + 0.01 * r.standard_normal((n + m, d))
    y = np.where(lab % 2 == 0, 1.0, -1.0)
    return Z[:n], y[:n], Z[n:]


def fit_args(leaf, rel_tol, extra=()):
    return ["--hss_leaf_size", str(leaf), "--hss_rel_tol", str(rel_tol)] + list(extra)


def dense_residual(kr, X, y, h, lam):
    """|(K + lambda I) w - y| / |y| with K formed in numpy on the cluster-ordered points"""
    perm = kr.permutation() - 1
    Xp, yp = X[perm], y[perm]
    Kd = KC.kernel_np(Xp, np.arange(len(Xp)), np.arange(len(Xp)), 0, h, lam)
    return float(np.linalg.norm(Kd @ kr.weights() - yp) / np.linalg.norm(yp)), Xp


def case_capi_end_to_end(KM, lib, d, rel_tol, n=2000, m=20, leaf=128, device=False):
    """Gauss kernel ridge regression in R^d through STRUMPACK_kernel_fit_HSS / _predict, double and float:
      * the double API with the default (device, exact) neighbour search compresses, and its dense residual r_dev is at most twice
        that of a fit with --hss_neighbor_search ann (the host search, which never depended on d): exact lists can only improve
        the column sample, the factor 2 covers the sampling difference;
      * its prediction agrees with numpy's w @ k under the bound of kernel_cases.case_kernel_predict;
      * the float API on float32(X) equals the double API on the widened floats: permutation, node table, weights after one
        rounding; its prediction meets the bound of DESIGN.md 8b with no matrix-core tile;
      * device=True: SPX_kernel_predict_device_float equals the host-pointer call bit for bit.
    Returns (r_dev, r_ann)."""
    h, lam = PC.f32(np.sqrt(d)), 1.0     # (float-representable: the float and the double entry points get the same width)
    X, y, T = clustered_points(1000 + d, n, m, d)
    kw = dict(h=h, lam=lam, kernel="Gauss", argv=fit_args(leaf, rel_tol))
    kd = KM.KernelRegression(lib, **kw).fit(X, y)
    ka = KM.KernelRegression(lib, h=h, lam=lam, kernel="Gauss", argv=fit_args(leaf, rel_tol, ["--hss_neighbor_search", "ann"])).fit(X, y)
    Xf, yf, Tf = X.astype(np.float32), y.astype(np.float32), T.astype(np.float32)
    kf = KM.KernelRegression(lib, **kw).fit(Xf, yf)
    kw_ = KM.KernelRegression(lib, **kw).fit(Xf.astype(np.float64), yf.astype(np.float64))
    try:
        info = kd.info()
        assert info["compressed"] == 1 and info["levels"] >= 3, info
        # (compressed: the largest rank stays below the n / 2 columns of the root's off-diagonal blocks)
        assert 0 < info["rank"] < n // 2, info
        r_dev, Xp = dense_residual(kd, X, y, h, lam)
        r_ann, _ = dense_residual(ka, X, y, h, lam)
        print("kernel ridge regression d=%d n=%d rel_tol=%g: rank %d (ann %d), dense residual r_dev %.3e r_ann %.3e" %
              (d, n, rel_tol, info["rank"], ka.info()["rank"], r_dev, r_ann))
        assert r_dev <= 2 * r_ann, (r_dev, r_ann)
        # FP64 prediction against the long double sum
        w = kd.weights()
        pd = kd.decision_function(T)
        Zall = np.vstack([Xp, T])
        k, a, A = KC.kernel_ref(Zall, np.arange(n), n + np.arange(m), 0, h, 0.0)
        aw = np.abs(w).astype(np.longdouble)
        bound = aw @ KC.kernel_entry_bound(a, A, 0, d, 0.0) + n * KC.U53 * (aw @ np.abs(k))
        err = np.abs(pd.astype(np.longdouble) - w.astype(np.longdouble) @ k)
        assert np.all(err <= bound), "STRUMPACK_kernel_predict_double: worst %.3g x the bound" % float((err / bound).max())
        # float API == double API on the widened floats
        perm = kf.permutation()
        assert np.array_equal(perm, kw_.permutation()), "permutation"
        assert np.array_equal(kf.node_info(), kw_.node_info()), "node table"
        fi, di = kf.info(), kw_.info()
        for key in ("compressed", "levels", "rank", "memory", "neighbors"):
            assert fi[key] == di[key], (key, fi[key], di[key])
        wf, wd = kf.weights(), kw_.weights()
        assert wf.dtype == np.float32
        assert np.array_equal(wf.view(np.uint32), wd.astype(np.float32).view(np.uint32)), "float weights != float32(double weights)"
        assert np.array_equal(kf.X_, Xf[perm - 1]), "the caller's array is not in cluster order"
        pf = kf.decision_function(Tf)
        st = kf.predict_stats()
        P, B = PC.reference(kf.X_, Tf, wf, 0, h, 1)
        ef = np.abs(pf.astype(np.float64) - P)
        print("  float prediction: largest error / bound %.3f; tiles mfma %d diff %d" % (float((ef / B).max()), st["mfma_tiles"], st["diff_tiles"]))
        assert np.all(ef <= B), "STRUMPACK_kernel_predict_float beyond the bound"
        assert st["mfma_tiles"] == 0 and st["diff_tiles"] == (-(-n // 64)) * (-(-m // 64)), st
        if device:
            import torch
            pt = kf.decision_function(torch.from_numpy(Tf).cuda())
            assert pt.is_cuda and np.array_equal(pt.cpu().numpy().view(np.uint32), pf.view(np.uint32)), "device entry differs from the host entry"
        return r_dev, r_ann
    finally:
        for kk in (kd, ka, kf, kw_):
            kk.destroy()



# ---- the reference's own fit in R^100 (tests/golden/kernel_highdim_golden.*, made by tests/golden/make_golden_kernel_highdim.py) --
_golden = {}


def highdim_golden():
    import json
    if not _golden:
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        _golden["json"] = json.load(open(os.path.join(gold, "kernel_highdim_golden.json")))
        _golden["npz"] = dict(np.load(os.path.join(gold, "kernel_highdim_golden.npz")))
    return _golden["json"], _golden["npz"]


def case_reference_fixture(KM, lib, ann):
    """Gauss kernel ridge regression on the fixture's 1500 points in R^100 against the reference's own permutation, node table,
    weights and predictions.
      ann=True: --hss_neighbor_search ann, the reference's randomized search on the host -> the reference's pipeline from the raw
        points: same permutation, per-node ranks equal (one off on at most 10 % of the nodes: LAPACK against device rounding at
        the cut), weights and predictions to 1e-6;
      ann=False: the exact device search beyond R^64 -> another column sample: the allowances of
        tests/test_kernel_gpu.py::test_regression_with_device_neighbours (largest rank within 15 %, weights 2e-2)."""
    import kernel_golden as KG
    g, Z = highdim_golden()
    X, y, T = Z["X"].astype(np.float64), Z["y"].astype(np.float64), Z["T"].astype(np.float64)
    kr = KM.KernelRegression(lib, h=g["h"], lam=g["lam"], kernel="Gauss", degree=g["p"],
                             argv=KG.fit_args(g) + (["--hss_neighbor_search", "ann"] if ann else [])).fit(X, y)
    try:
        info = kr.info()
        assert info["compressed"] == 1 == g["compressed"]
        assert np.array_equal(kr.permutation(), Z["perm"]), "cluster permutation differs from the reference's"
        nodes, ref = kr.node_info(), np.array(g["nodes"])
        assert nodes.shape == ref.shape and np.array_equal(nodes[:, [0, 1, 5]], ref[:, [0, 1, 5]]), "tree shape"
        dr = np.abs(nodes[:, 3] - ref[:, 3])
        w, wr = kr.weights(), Z["weights"]
        pred, pr = kr.decision_function(T), Z["prediction"]
        ew, ep = np.linalg.norm(w - wr) / np.linalg.norm(wr), np.linalg.norm(pred - pr) / np.linalg.norm(pr)
        print("reference fixture d=%d (%s neighbours): rank %d (reference %d), nodes with another rank %d of %d (largest difference "
              "%d), weights %.3e, predictions %.3e" % (g["d"], "ann" if ann else "device", info["rank"], g["rank"], int((dr > 0).sum()),
                                                      len(dr), int(dr.max()), ew, ep))
        if ann:
            assert dr.max() <= 1 and (dr > 0).mean() <= 0.1, (nodes[:, 3], ref[:, 3])
            assert abs(info["rank"] - g["rank"]) <= 1, (info["rank"], g["rank"])
            assert ew <= 1e-6 and ep <= 2e-6, (ew, ep)
        else:
            assert abs(info["rank"] - g["rank"]) <= 0.15 * g["rank"] + 1, (info["rank"], g["rank"])
            assert ew <= 2e-2 and ep <= 2 * 2e-2, (ew, ep)
        return ew
    finally:
        kr.destroy()
