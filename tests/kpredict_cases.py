"""Checks of the single-precision kernel ridge regression path shared by the GPU tests (product library) and the CPU tests
(the same sources on the fiber emulator): hssk_kernel_predict_f32 against FP64 numpy under the error bound derived in
DESIGN.md ("Single-precision prediction"), and the STRUMPACK_*_float entry points pinned to the double ones on the same data.

The bound, per test point c (u = 2^-24, P_c the FP64 value on the widened float inputs, a_rc >= 0 the exponent's magnitude,
mu the training mean, q_rc = (|x_r - mu|^2 + |t_c - mu|^2) / (2 h^2)):
  Gauss    |pred_c - P_c| <= sum_r |w_r| k_rc [u (64 + (d + 4) a_rc) + min(4 (d + 4) u q_rc, 2^-13)] + u |P_c|
  Laplace  the same without the min(...) term
  ANOVA    |pred_c - P_c| <= sum_r |w_r| A_rc u (64 + p (d + 10 + 5 amax_rc)) + u |P_c|,  A_rc = the recurrence with all signs
           positive (>= |k_rc|), amax_rc the largest per-coordinate exponent of the pair
all three plus the underflow floor 2^-126 (1 + sum_r |w_r|): kernel values below the FP32 normal range have no relative accuracy.
"""
import numpy as np

U = 2.0 ** -24
TAU = 2.0 ** -13
TILE = 64


def reference(X, T, w, ktype, h, p=1):
    """FP64 value P (m) and the bound B (m) for float32 X (n x d), T (m x d), w (n)"""
    X64, T64, w64 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (X, T, w))
    n, d = X64.shape
    m = T64.shape[0]
    P, B = np.zeros(m), np.zeros(m)
    if n == 0 or m == 0:
        return P, B
    block = int(max(1, min(256, 10_000_000 // (n * d))))    # (test points per pass: the n x block x d differences stay small)
    mu = X64.mean(0)
    aw = np.abs(w64)
    nx = ((X64 - mu) ** 2).sum(1)
    for c0 in range(0, m, block):
        Tb = T64[c0:c0 + block]
        df = X64[:, None, :] - Tb[None, :, :]                       # n x b x d
        if ktype == 0:
            a = (df ** 2).sum(-1) / (2 * h * h)
            k = np.exp(-a)
            q = (nx[:, None] + ((Tb - mu) ** 2).sum(1)[None, :]) / (2 * h * h)
            rel = U * (64 + (d + 4) * a) + np.minimum(4 * (d + 4) * U * q, TAU)
            kabs = k
        elif ktype == 1:
            a = np.abs(df).sum(-1) / h
            k = np.exp(-a)
            rel = U * (64 + (d + 4) * a)
            kabs = k
        else:
            ai = df ** 2 / (2 * h * h)
            t = np.exp(-ai)
            Kss = [(t ** (j + 1)).sum(-1) for j in range(p)]
            Kpp, App = [np.ones(t.shape[:2])], [np.ones(t.shape[:2])]
            for i in range(1, p + 1):
                Kpp.append(sum((-1) ** (s + 1) * Kpp[i - s] * Kss[s - 1] for s in range(1, i + 1)) / i)
                App.append(sum(App[i - s] * Kss[s - 1] for s in range(1, i + 1)) / i)
            k, kabs = Kpp[p], App[p]
            rel = U * (64 + p * (d + 10 + 5 * ai.max(-1)))
        P[c0:c0 + block] = w64 @ k
        B[c0:c0 + block] = aw @ (kabs * rel)
    # FP32 range: a term below the smallest normal number 2^-126 is accurate to that absolutely, not relatively (it may be
    # flushed to zero), and so is the float result itself
    return P, B + U * np.abs(P) + 2.0 ** -126 * (aw.sum() + 1)


def splits_expected(n, m):
    """the split rule of hssk_kernel_predict_f32 (a function of (n, m) alone): chunks of 4 x 64 training points, as many splits
    as bring the grid to 2048 workgroups, at most one per chunk"""
    if n <= 0 or m <= 0:
        return 0
    chunks, nt = -(-n // 256), -(-m // TILE)
    return max(1, min(-(-2048 // nt), chunks))


def check_predict(hk, X, T, w, ktype, h, p=1, tag="", routes=None):
    """one call checked against the bound, a second one for bitwise equality; routes: None, 'mfma' (matrix-core tiles only),
    'diff' (difference-form tiles only) or 'both'.  Returns (largest error / bound, statistics)."""
    X, T, w = (np.ascontiguousarray(a, dtype=np.float32) for a in (X, T, w))
    n, m = X.shape[0], T.shape[0]
    out, st = hk.kernel_predict_f32(X, w, T, ktype, h, p, stats=True)
    out2 = hk.kernel_predict_f32(X, w, T, ktype, h, p)
    assert out.dtype == np.float32 and out.shape == (m,)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), tag + ": two runs differ"
    P, B = reference(X, T, w, ktype, h, p)
    err = np.abs(out.astype(np.float64) - P)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = float(np.nanmax(np.where(B > 0, err / B, 0.0))) if m else 0.0
    print("%s type=%d n=%d m=%d d=%d: largest error / bound %.3f, tiles mfma %d diff %d, splits %d" %
          (tag, ktype, n, m, X.shape[1], frac, st[0], st[1], st[2]))
    assert np.all(err <= B), tag + ": %d predictions beyond the bound (worst %.3g x)" % (int((err > B).sum()), frac)
    if m and n:
        assert st[0] + st[1] == (-(-n // TILE)) * (-(-m // TILE)), (tag, st)
        assert st[2] == splits_expected(n, m) == hk.lib.hssk_kernel_predict_splits(n, m), (tag, st)
    if ktype != 0:
        assert st[0] == 0
    if routes == "mfma":
        assert st[1] == 0 and st[0] > 0, (tag, st)
    elif routes == "diff":
        assert st[0] == 0 and st[1] > 0, (tag, st)
    elif routes == "both":
        assert st[0] > 0 and st[1] > 0, (tag, st)
    return frac, st


def points(seed, n, m, d):
    r = np.random.default_rng(seed)
    return (r.standard_normal((n, d)).astype(np.float32), r.standard_normal((m, d)).astype(np.float32),
            r.standard_normal(n).astype(np.float32))


def case_types_and_dimensions(hk, d, n=257, m=70):
    """all three kernels at dimension d, ragged n and m; the Gauss width grows with sqrt(d) so that the tiles of a standard
    normal cloud pass the route rule (the matrix-core variant of every d is exercised)"""
    X, T, w = points(100 + d, n, m, d)
    check_predict(hk, X, T, w, 0, 0.9 * np.sqrt(d) + 0.4, tag="gauss d=%d" % d, routes="mfma")
    check_predict(hk, X, T, w, 0, 0.35, tag="gauss narrow d=%d" % d)
    check_predict(hk, X, T, w, 1, 0.9 * d, tag="laplace d=%d" % d, routes="diff")
    for p in sorted({1, min(2, d), min(8, d)}):
        check_predict(hk, X, T, w, 2, 1.1, p, tag="anova p=%d d=%d" % (p, d), routes="diff")


def case_small_and_empty(hk):
    X, T, w = points(7, 40, 70, 5)           # n below one tile
    check_predict(hk, X, T, w, 0, 1.3, tag="n<tile", routes="mfma")
    check_predict(hk, X, T[:1], w, 0, 1.3, tag="m=1")
    check_predict(hk, X, T[:1], w, 1, 1.3, tag="m=1 laplace")
    check_predict(hk, X[:1], T, w[:1], 2, 1.3, 2, tag="n=1 anova")
    out, st = hk.kernel_predict_f32(X, w, T[:0], 0, 1.3, stats=True)   # m == 0: nothing launched
    assert out.shape == (0,) and not st.any()
    out = hk.kernel_predict_f32(X[:0], w[:0], T, 0, 1.3)               # no training points: zeros
    assert np.array_equal(out, np.zeros(70, dtype=np.float32))


def case_splits(hk, sizes):
    """sizes: (n, m, expected splits) -- one, two and many splits of the training set"""
    for n, m, s in sizes:
        assert splits_expected(n, m) == s, (n, m, splits_expected(n, m))
        X, T, w = points(n + m, n, m, 8)
        _, st = check_predict(hk, X, T, w, 0, 1.3 * 2, tag="splits=%d" % s)
        assert st[2] == s
        check_predict(hk, X, T, w, 1, 4.0, tag="splits=%d laplace" % s)


def case_offset(hk, n=300, m=70):
    """every coordinate offset by 1e4: the centring keeps the norm expansion usable"""
    r = np.random.default_rng(5)
    X = (r.random((n, 8)) + 1e4).astype(np.float32)
    T = (r.random((m, 8)) + 1e4).astype(np.float32)
    w = r.standard_normal(n).astype(np.float32)
    for kt, p in ((0, 1), (1, 1), (2, 2)):
        check_predict(hk, X, T, w, kt, 1.3, p, tag="offset 1e4", routes="mfma" if kt == 0 else "diff")


def case_bimodal(hk, n=300, m=130):
    """two Gaussian clusters at +-1000: every tile is far from the mean, none may take the norm expansion"""
    r = np.random.default_rng(6)
    sx, stt = np.where(r.random(n) < 0.5, 1000.0, -1000.0), np.where(r.random(m) < 0.5, 1000.0, -1000.0)
    X = (r.standard_normal((n, 8)) + sx[:, None]).astype(np.float32)
    T = (r.standard_normal((m, 8)) + stt[:, None]).astype(np.float32)
    w = r.standard_normal(n).astype(np.float32)
    check_predict(hk, X, T, w, 0, 1.3, tag="bimodal", routes="diff")


def case_outliers(hk, n=700, m=200):
    """a few far outliers among the training and the test points: their tiles go the difference form, the others stay on the
    matrix cores"""
    r = np.random.default_rng(8)
    X = r.random((n, 8)).astype(np.float32)
    T = r.random((m, 8)).astype(np.float32)
    X[[3, 500]] += 300.0
    T[150] -= 200.0
    w = r.standard_normal(n).astype(np.float32)
    check_predict(hk, X, T, w, 0, 1.3, tag="outliers", routes="both")


def case_errors(hk):
    X, T, w = points(1, 64, 10, 4)
    dX, dT, dw, dp = hk.array(X.ravel()), hk.array(T.ravel()), hk.array(w), hk.empty((10,), np.float32)
    f = hk.lib.hssk_kernel_predict_f32

    def call(X=dX.ptr, n=64, d=4, kt=0, p=1, h=1.0, w=dw.ptr, T=dT.ptr, m=10, out=dp.ptr):
        return f(hk.ctx, X, n, d, kt, p, h, w, T, m, out, None)
    assert call() == 0
    for kw, word in ((dict(d=65), "dimension"), (dict(d=0), "dimension"), (dict(kt=3), "type"), (dict(kt=2, p=9), "degree"),
                     (dict(kt=2, p=5), "degree"), (dict(kt=2, p=0), "degree"), (dict(X=None), "null"), (dict(w=None), "null"),
                     (dict(T=None), "null"), (dict(out=None), "null"), (dict(n=-1), "range"), (dict(m=-1), "range"),
                     (dict(n=1 << 40), "range"), (dict(h=0.0), "width")):
        assert call(**kw) != 0, kw
        assert word in hk.error(), (kw, hk.error())
    assert call(m=0, T=None, out=None) == 0
    hk.sync()
    for a in (dX, dT, dw, dp):
        a.free()


# ---- the float C interface against the double one ---------------------------------------------------------------------------
def f32(v):
    return float(np.float32(v))


def fit_pair(KM, lib, tag, inject):
    """the float API on Xf = float32(X) and the double API on the widened Xf, same options (h and lambda float-representable)"""
    import kernel_golden as KG
    J, Z = KG.golden()
    g = J["regression_" + tag]
    X, y, T, yt = KG.susy()
    n, m = g["n"], g["m"]
    Xf, yf, Tf = X[:n].astype(np.float32), y[:n].astype(np.float32), T[:m].astype(np.float32)
    kw = dict(h=f32(g["h"]), lam=f32(g["lam"]), kernel=KG.KERNEL_NAME[g["ktype"]], degree=g["p"], argv=KG.fit_args(g))
    nb = Z["ann_" + tag] if inject else None
    kf = KM.KernelRegression(lib, **kw).fit(Xf, yf, neighbors=nb)
    kd = KM.KernelRegression(lib, **kw).fit(Xf.astype(np.float64), yf.astype(np.float64), neighbors=nb)
    return g, Z, Xf, yf, Tf, kf, kd


def check_sign(pred, P, B, tag):
    sure = np.abs(P) > B
    assert np.array_equal(pred[sure] >= 0, P[sure] >= 0), tag + ": a sign differs beyond the bound"
    assert (~sure).mean() <= 0.01, tag + ": %.2f %% of the test points are within the bound of zero" % (100 * (~sure).mean())


def check_float_vs_double(KM, lib, tag, inject):
    g, Z, Xf, yf, Tf, kf, kd = fit_pair(KM, lib, tag, inject)
    try:
        perm = kf.permutation()
        assert np.array_equal(perm, kd.permutation()), "permutation"
        assert np.array_equal(kf.node_info(), kd.node_info()), "node table"
        fi, di = kf.info(), kd.info()
        for key in ("compressed", "levels", "rank", "memory", "neighbors"):
            assert fi[key] == di[key], (key, fi[key], di[key])
        wf, wd = kf.weights(), kd.weights()
        assert wf.dtype == np.float32 and wd.dtype == np.float64
        assert np.array_equal(wf.view(np.uint32), wd.astype(np.float32).view(np.uint32)), "float weights != float32(double weights)"
        assert np.array_equal(kf.X_, Xf[perm - 1]), "the caller's array is not in cluster order"
        assert np.array_equal(kf.y_, yf[perm - 1]), "the caller's labels are not in cluster order"
        pf = kf.decision_function(Tf)
        assert pf.dtype == np.float32
        st = kf.predict_stats()
        P, B = reference(kf.X_, Tf, wf, g["ktype"], f32(g["h"]), g["p"])
        err = np.abs(pf.astype(np.float64) - P)
        print("%s inject=%s: largest error / bound %.3f; tiles mfma %d diff %d" % (tag, inject, float((err / B).max()), st["mfma_tiles"], st["diff_tiles"]))
        assert np.all(err <= B), tag
        check_sign(pf, P, B, tag)
        # the double API's prediction: its weights differ from the float ones by one rounding (u |w_r| per term), its sums are FP64
        pd = kd.decision_function(Tf.astype(np.float64))
        S, _ = reference(kf.X_, Tf, np.abs(wd), g["ktype"], f32(g["h"]), g["p"])     # sum_r |w_r| k_rc (k > 0 for all three kernels)
        assert np.all(np.abs(pf.astype(np.float64) - pd) <= B + 1.01 * U * S + 1e-12 * S), tag + ": against the double API"
    finally:
        kf.destroy()
        kd.destroy()


# (prediction, weights) tolerances against the reference's fixtures: four times the deviations measured on the device
# (profiles/f32_predict.md), to cover emulator-versus-device rounding
# measured on the MI355X (prediction, weights): gauss_400 2.597e-7, 4.204e-8; laplace_400 1.232e-7, 4.014e-8; gauss_1500 3.396e-7, 4.519e-8
# (the double path's own 2 w_tol for these tags is 2e-7)
FIXTURE_TOL = {"gauss_400": (4 * 2.597e-7, 4 * 4.204e-8), "laplace_400": (4 * 1.232e-7, 4 * 4.014e-8),
               "gauss_1500": (4 * 3.396e-7, 4 * 4.519e-8)}


def check_float_vs_fixture(KM, lib, tag, pred_tol, w_tol):
    """the float API with the reference's neighbour lists against the reference's own numbers (made from double data):
    permutation equal, ranks one off on at most a tenth of the nodes; weights and predictions to the tolerances measured on
    the device (profiles/f32_predict.md) times four.  Returns the measured (weights, prediction) deviations."""
    import kernel_golden as KG
    J, Z = KG.golden()
    g = J["regression_" + tag]
    X, y, T, yt = KG.susy()
    n, m = g["n"], g["m"]
    kf = KM.KernelRegression(lib, h=g["h"], lam=g["lam"], kernel=KG.KERNEL_NAME[g["ktype"]], degree=g["p"], argv=KG.fit_args(g))
    kf.fit(X[:n].astype(np.float32), y[:n].astype(np.float32), neighbors=Z["ann_" + tag])
    try:
        assert np.array_equal(kf.permutation(), Z["perm_" + tag]), "cluster permutation differs from the reference's"
        nodes, ref = kf.node_info(), np.array(g["nodes"])
        assert nodes.shape == ref.shape and np.array_equal(nodes[:, [0, 1, 5]], ref[:, [0, 1, 5]]), "tree shape"
        dr = np.abs(nodes[:, 3] - ref[:, 3])
        assert dr.max() <= 1 and (dr > 0).mean() <= 0.1, (nodes[:, 3], ref[:, 3])
        wr, pr = Z["weights_" + tag], Z["prediction_" + tag]
        ew = float(np.linalg.norm(kf.weights() - wr) / np.linalg.norm(wr))
        perm = Z["perm_" + tag]
        d = X.shape[1]
        quirk = any(perm[i] <= d and perm[i] != i + 1 for i in range(min(d, n)))   # (tests/kernel_golden.py: Kernel::permute())
        pred = kf.decision_function(T[:m].astype(np.float32)).astype(np.float64)
        if quirk:
            pr, _ = reference(X[:n][perm - 1], T[:m], wr, g["ktype"], g["h"], g["p"])
        ep = float(np.linalg.norm(pred - pr) / np.linalg.norm(pr))
        print("%s: float API against the reference fixture: weights %.3e, prediction %.3e%s" % (tag, ew, ep, " (formula: permute() quirk)" if quirk else ""))
        assert ew <= w_tol, (tag, ew)
        assert ep <= pred_tol, (tag, ep)
        return ew, ep
    finally:
        kf.destroy()


def check_resident_and_device_entry(KM, lib):
    """GPU: the model stays resident, the device entry equals the host entry bit for bit and refuses what it cannot take"""
    import torch
    g, Z, Xf, yf, Tf, kf, kd = fit_pair(KM, lib, "gauss_400", True)
    try:
        m, d = Tf.shape
        p1 = kf.decision_function(Tf)
        s1 = kf.predict_stats()
        p2 = kf.decision_function(Tf)
        s2 = kf.predict_stats()
        assert s1["resident"] == 1 and s2["resident"] == 1, (s1, s2)     # the fit left the model in HBM
        assert s1["uploaded_bytes"] == 4 * d * m and s2["uploaded_bytes"] == 4 * d * m, (s1, s2)
        assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
        tT = torch.from_numpy(Tf).cuda()
        pt = kf.decision_function(tT)
        assert pt.is_cuda and pt.dtype == torch.float32
        s3 = kf.predict_stats()
        assert s3["uploaded_bytes"] == 0 and s3["resident"] == 1, s3
        assert np.array_equal(pt.cpu().numpy().view(np.uint32), p1.view(np.uint32)), "device entry differs from the host entry"
        out = np.zeros(m, dtype=np.float32)
        tout = torch.empty(m, dtype=torch.float32, device="cuda")
        assert lib.SPX_kernel_predict_device_float(kf.K, m, Tf.ctypes.data, tout.data_ptr()) != 0      # host test points
        assert lib.SPX_kernel_predict_device_float(kf.K, m, tT.data_ptr(), out.ctypes.data) != 0       # host output
        assert lib.SPX_kernel_predict_device_float(kd.K, m, tT.data_ptr(), tout.data_ptr()) != 0       # double handle
        st = np.zeros(6, dtype=np.int64)
        assert lib.SPX_kernel_predict_stats(kd.K, st.ctypes.data) != 0
    finally:
        kf.destroy()
        kd.destroy()


def check_lifecycle(KM, lib):
    """destroy after fit, fit twice on one object, predict before fit (an error, no crash)"""
    import kernel_golden as KG
    X, y, T, yt = KG.susy()
    Xf, yf, Tf = X[:200].astype(np.float32), y[:200].astype(np.float32), T[:50].astype(np.float32)
    args = ["--hss_leaf_size", "32", "--hss_approximate_neighbors", "64"]
    K = lib.STRUMPACK_create_kernel_float(200, 8, Xf.copy().ctypes.data, 1.3, 3.11, 1, 0)
    assert K
    out = np.full(50, 7.0, dtype=np.float32)
    lib.STRUMPACK_kernel_predict_float(K, 50, Tf.ctypes.data, out.ctypes.data)     # before a fit: reported, nothing written
    assert np.all(out == 7.0)
    w = np.zeros(200)
    assert lib.SPX_kernel_weights(K, w.ctypes.data) != 0
    lib.STRUMPACK_destroy_kernel_float(K)
    kr = KM.KernelRegression(lib, h=1.3, lam=3.11, kernel="rbf", argv=args)
    kr.fit(Xf, yf)
    p1 = kr.decision_function(Tf)
    kr.fit(Xf, yf)            # (a second fit on the same object: the first handle is destroyed with its resident model)
    p2 = kr.decision_function(Tf)
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    kr.destroy()              # destroy right after a fit + prediction
    kr = KM.KernelRegression(lib, h=1.3, lam=3.11, kernel="rbf", argv=args).fit(Xf, yf)
    kr.destroy()              # destroy after a fit, no prediction
    # a float64 fit stays on the double entry points
    kd = KM.KernelRegression(lib, h=1.3, lam=3.11, kernel="rbf", argv=args).fit(Xf.astype(np.float64), yf)
    assert kd.weights().dtype == np.float64 and kd.decision_function(Tf).dtype == np.float64
    kd.destroy()
