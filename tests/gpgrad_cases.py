"""Checks of the gradient of the log marginal likelihood from a kept kernel ridge regression fit: hssk_kernel_matmul, hssk_coldots,
Kernel<double>::log_marginal_likelihood_gradient / model_probes / model_residual and their C and Python forms.  Shared by the CPU
emulator tests (tests/test_gpgrad_emu.py) and the GPU tests (tests/test_gpgrad_gpu.py), as tests/gp_cases.py is.

The formulas.  H = K + lambda I, alpha = H^-1 y, L = -1/2 y^T alpha - 1/2 log|det H| - n/2 log 2 pi,
    dL/dtheta = 1/2 alpha^T (dH/dtheta) alpha - 1/2 tr(H^-1 dH/dtheta),
dH/dlambda = I, dK/dh = K' with K'_ij = k_ij |x_i - x_j|_2^2 / h^3 (Gauss), k_ij |x_i - x_j|_1 / h^2 (Laplace).  check_oracle compares
them with central differences of L in plain numpy on dense matrices: the formulas themselves, no library code.

The product kernel.  The reference is kernel_cases.kernel_ref in long double: k, and a, the magnitude of the exponent.  The
derivative is g = k a c_h with c_h = 2 / h (Gauss), 1 / h (Laplace).  An entry of the product is a sum over the training points,
    |out(i, c) - ref(i, c)| <= sum_r (b'_ir + n u |g_ir|) |B(r, c)|,    u = 2^-53,
b' the error bound of one evaluated entry of g and n u |g| the rounding of the n-term sum (the matrix cores add four products at
a time into an FP64 accumulator: at most n roundings per entry, also when split partials are added afterwards).
  deriv = 0:  b' = kernel_entry_bound(a, A, type, d, lambda) = u (8 + (d + 4) a) k + u |lambda|.
  deriv = 1:  the kernel computes e^ = fl(acc scale), k^ = exp(e^) and g^ = fl(fl(k^ (-e^)) c_h^).  k^ is within b =
              kernel_entry_bound(.., lambda = 0) of k; -e^ is a (1 + delta) with |delta| <= (d + 4) u (what kernel_entry_bound
              itself assumes of the d-term sum and its scaling); the two products and the rounding of c_h add at most 3 u.  To
              first order |g^ - g| <= c_h (a b + (d + 7) u a k).  The form asserted is
                  b' = c_h (a b + (d + 6) u a k):
              a b carries 8 u a k for the exponential and its argument where the exponential is within one unit in the last
              place (2 u), so the u a k missing in the second term is covered more than five times over.
The duplicate points of check_matmul_properties have a = 0 exactly, so g = 1 * 0 * c_h = 0 exactly.

hssk_coldots.  n products, each rounded, added in some fixed order: |got - ref| <= n u sum_i |a_i b_i|.

The gradient of a kept model.  Hd is the dense form of the matrix the handle writes (gp_cases.dense_model), X, y, alpha the
handle's points, labels and weights, Z an explicit block of probes in cluster order.  Reference: s = solve(Hd, Z), g = K' Z with
the long double K', th_k = s_k^T g_k, tl_k = s_k^T z_k, quad_h = 1/2 alpha^T K' alpha, quad_lambda = 1/2 alpha^T alpha.  The library
solves with the ULV factors, s^ = s + delta, ||delta_k|| <= EPS_F cond_2(Hd) ||s_k|| (the forward error the project accepts,
gp_cases.EPS_F = 1e-12), and multiplies with the evaluated kernel, g^ = g + e, |e_ik| <= E_ik, E the product bound above.  Hence
    |th^_k - th_k| <= EPS_F cond_2(Hd) ||s_k|| ||g_k|| + sum_i |s_ik| E_ik,
    |tl^_k - tl_k| <= EPS_F cond_2(Hd) ||s_k|| ||z_k||                          (no product),
    |quad_h^ - quad_h| <= 1/2 sum_i |alpha_i| E_i(alpha)                         (no solve),
(the rounding of the n-term dot products, n u ||s|| ||g||, is below the first term: n u < 1e-12, as in gp_cases).  quad_lambda is
a long double sum on both sides: 4 u quad_lambda.  The traces are the means of the per-probe values and inherit the means of
their bounds, dh = quad_h - trace_h / 2 and dlambda = quad_lambda - trace_lambda / 2 the sums.  A case only proves something
while the bound of dh is small against the two terms it is the difference of: every case asserts
    bound(dh) <= 1e-4 min(|trace_h|, |quad_h|).

The residual ||y - (K + lambda I) alpha|| / ||y|| differs from its long double reference by at most ||E(alpha)||_2 / ||y||_2 (the
triangle inequality on the numerator), E(alpha) the deriv = 0 product bound of the alpha column."""
import ctypes

import numpy as np

import gp_cases as GP
import kernel_cases as KC
from strumpack_amd import hssk as K

LD = np.longdouble
U = KC.U53
KT = {"gauss": 0, "laplace": 1}


# ---- 1. the formulas themselves ---------------------------------------------------------------------------------------------------
def dense_lml(X, y, ktype, h, lam):
    Kd = KC.kernel_np(X, np.arange(len(X)), np.arange(len(X)), ktype, h, lam)
    alpha = np.linalg.solve(Kd, y)
    return -0.5 * y @ alpha - 0.5 * np.linalg.slogdet(Kd)[1] - 0.5 * len(X) * np.log(2.0 * np.pi)


def dense_gradient(X, y, ktype, h, lam):
    n = len(X)
    idx = np.arange(n)
    Kd = KC.kernel_np(X, idx, idx, ktype, h, 0.0)
    df = X[:, None, :] - X[None, :, :]
    Kp = Kd * ((df ** 2).sum(-1) / h ** 3 if ktype == 0 else np.abs(df).sum(-1) / h ** 2)
    Hi = np.linalg.inv(Kd + lam * np.eye(n))
    alpha = Hi @ y
    return 0.5 * alpha @ Kp @ alpha - 0.5 * np.trace(Hi @ Kp), 0.5 * alpha @ alpha - 0.5 * np.trace(Hi)


def check_oracle(kern, d, n=200, lam=4.0, step=1e-5):
    """analytic gradient of the dense L against central differences with step 1e-5: relative agreement within 1e-5 (truncation
    step^2 L''' / 6 and cancellation u |L| / step are both below 1e-8 of the gradients here)"""
    X, y, _ = GP.model_data(d, n, 2)
    ktype = KT[kern]
    h = float(KC.kernel_widths(d)[ktype])
    dh, dl = dense_gradient(X, y, ktype, h, lam)
    fh = (dense_lml(X, y, ktype, h + step, lam) - dense_lml(X, y, ktype, h - step, lam)) / (2 * step)
    fl = (dense_lml(X, y, ktype, h, lam + step) - dense_lml(X, y, ktype, h, lam - step)) / (2 * step)
    print("oracle %s R^%d: dL/dh %.9g (differences %.9g), dL/dlambda %.9g (differences %.9g)" % (kern, d, dh, fh, dl, fl))
    assert abs(dh - fh) <= 1e-5 * abs(dh), (dh, fh)
    assert abs(dl - fl) <= 1e-5 * abs(dl), (dl, fl)


# ---- 2. hssk_kernel_matmul on its own ---------------------------------------------------------------------------------------------
def g_reference(X, ktype, h, d, deriv, lam):
    """(g, b') in long double over all pairs of the rows of X: the matrix the product is taken with and its entry bound"""
    idx = np.arange(len(X))
    if deriv == 0:
        k, a, A = KC.kernel_ref(X, idx, idx, ktype, h, lam)
        return k, KC.kernel_entry_bound(a, A, ktype, d, lam)
    k, a, A = KC.kernel_ref(X, idx, idx, ktype, h, 0.0)
    ch = (LD(2) if ktype == 0 else LD(1)) / LD(h)
    return k * a * ch, ch * (a * KC.kernel_entry_bound(a, A, ktype, d, 0.0) + (d + 6) * U * a * k)


def product_bound(g, bp, B):
    """E(i, c) = sum_r (b'_ir + n u |g_ir|) |B(r, c)|"""
    return (bp + len(g) * U * np.abs(g)) @ np.abs(B).astype(LD)


def matmul(hk, dX, n, d, ktype, h, lam, deriv, B, splits=0, pad=(3, 5)):
    """one call on a padded B into a pre-filled padded output: returns the n x nc result after checking the sentinels"""
    nc = B.shape[1]
    ldb, ldo = n + pad[0], n + pad[1]
    Bp = np.full((ldb, nc), 1e300)
    Bp[:n] = B
    dB, dO = hk.array(Bp), hk.array(np.full((ldo, nc + 1), KC.SENTINEL))
    spec = K.KernelSpec(dX.ptr, n, d, ktype, 1, h, lam)
    hk.check(hk.lib.hssk_kernel_matmul(hk.ctx, ctypes.byref(spec), deriv, dB.ptr, ldb, nc, dO.ptr, ldo, splits))
    hk.sync()
    got = dO.get()
    dB.free()
    dO.free()
    assert np.all(got[n:, :] == KC.SENTINEL) and np.all(got[:, nc] == KC.SENTINEL), "hssk_kernel_matmul wrote outside its block"
    return got[:n, :nc]


# (n, nc, d, kernel, deriv, splits, lambda): every n of {1, 15, 16, 17, 63, 64, 65, 130} (ragged row tiles and stages), every nc of
# {1, 16, 17, 64}, every d of {1, 8, 33, 64 (whole points in the LDS), 65, 70, 130 (chunks of 32 coordinates, ragged last chunk)},
# both kernels, both values of deriv, the splits forced to 1 and 3 at n = 130 (stages 48 + 48 + 34 points: a ragged last split)
MATMUL_CASES = [
    (1, 1, 1, "gauss", 0, 0, 0.0),
    (15, 16, 8, "laplace", 1, 0, 0.0),
    (16, 17, 33, "gauss", 1, 0, 0.0),
    (17, 64, 64, "laplace", 0, 0, 2.5),
    (63, 1, 65, "gauss", 1, 0, 0.0),
    (64, 16, 70, "laplace", 1, 0, 0.0),
    (65, 17, 130, "gauss", 0, 0, 0.7),
    (130, 64, 8, "gauss", 1, 1, 0.0),
    (130, 64, 8, "gauss", 1, 3, 0.0),
    (130, 17, 1, "laplace", 0, 3, 2.5),
    (130, 64, 65, "laplace", 1, 3, 0.0),
    (130, 16, 8, "gauss", 0, 1, 0.0),
]


def check_matmul(hk, n, nc, d, kern, deriv, splits, lam, seed=11):
    """the product against the long double reference under the bound of the module docstring; padded operands with sentinel rows;
    two calls bit for bit; splits = 0 bit for bit the forced hssk_kernel_matmul_splits(n)"""
    rng = np.random.default_rng(seed + n + d)
    X, B = rng.standard_normal((n, d)), rng.standard_normal((n, nc))
    ktype = KT[kern]
    h = float(KC.kernel_widths(d)[ktype])
    dX = hk.array(X.T)
    got = matmul(hk, dX, n, d, ktype, h, lam, deriv, B, splits)
    g, bp = g_reference(X, ktype, h, d, deriv, lam)
    ref, E = g @ B.astype(LD), product_bound(g, bp, B)
    err = np.abs(got.astype(LD) - ref)
    frac = float((err / E).max())
    print("kernel_matmul %s n=%d nc=%d d=%d deriv=%d splits=%d: largest error / bound %.3f" % (kern, n, nc, d, deriv, splits, frac))
    assert np.all(err <= E), (kern, n, nc, d, deriv, splits, frac)
    assert np.array_equal(got, matmul(hk, dX, n, d, ktype, h, lam, deriv, B, splits)), "two calls differ"
    auto = hk.lib.hssk_kernel_matmul_splits(n)
    assert auto >= 1
    assert np.array_equal(matmul(hk, dX, n, d, ktype, h, lam, deriv, B, 0), matmul(hk, dX, n, d, ktype, h, lam, deriv, B, auto)), "splits = 0"
    if deriv == 1:
        assert np.all(np.diag(np.asarray(g, dtype=np.float64)) == 0.0)
    dX.free()
    return frac


def check_matmul_properties(hk, seed=5):
    """duplicate points contribute exactly 0 to the derivative product; lambda on the diagonal is lambda B; padded leading
    dimensions may differ from each other"""
    rng = np.random.default_rng(seed)
    n, d, nc = 130, 8, 17
    for kern, ktype in KT.items():
        h = float(KC.kernel_widths(d)[ktype])
        X = rng.standard_normal((n, d))
        X[77] = X[3]
        X[129] = X[64]
        dX = hk.array(X.T)
        B = np.zeros((n, 4))
        B[77, 0], B[3, 1], B[129, 2], B[64, 3] = 1.5, -2.0, 3.0, 0.25
        for splits in (1, 3):
            got = matmul(hk, dX, n, d, ktype, h, 0.0, 1, B, splits)
            for col, (i, j) in enumerate([(3, 77), (77, 3), (64, 129), (129, 64)]):
                assert got[i, col] == 0.0 and got[j, col] == 0.0, (kern, splits, i, j, got[i, col], got[j, col])
            assert np.count_nonzero(got) == 4 * (n - 2)
        B = rng.standard_normal((n, nc))
        lam = 2.5
        g0, b0 = g_reference(X, ktype, h, d, 0, 0.0)
        g1, b1 = g_reference(X, ktype, h, d, 0, lam)
        with0, with1 = matmul(hk, dX, n, d, ktype, h, 0.0, 0, B), matmul(hk, dX, n, d, ktype, h, lam, 0, B)
        diff = np.abs(with1.astype(LD) - (with0.astype(LD) + LD(lam) * B.astype(LD)))
        assert np.all(diff <= product_bound(g0, b0, B) + product_bound(g1, b1, B)), kern
        assert not np.array_equal(with0, with1)
        dX.free()


def check_matmul_refusals(hk):
    n, d, nc = 40, 8, 5
    rng = np.random.default_rng(1)
    dX, dB = hk.array(rng.standard_normal((d, n))), hk.array(rng.standard_normal((n, 65)))
    fill = np.full((n, 65), KC.SENTINEL)
    dO = hk.array(fill)
    f = hk.lib.hssk_kernel_matmul
    ok = K.KernelSpec(dX.ptr, n, d, 0, 1, 1.3, 0.0)
    anova = K.KernelSpec(dX.ptr, n, d, 2, 2, 1.3, 0.0)
    empty = K.KernelSpec(dX.ptr, 0, d, 0, 1, 1.3, 0.0)
    assert f(hk.ctx, ctypes.byref(anova), 0, dB.ptr, n, nc, dO.ptr, n, 0) == 2 and "ANOVA" in hk.error()
    assert f(hk.ctx, ctypes.byref(anova), 1, dB.ptr, n, nc, dO.ptr, n, 0) == 2
    assert f(hk.ctx, ctypes.byref(ok), 1, dB.ptr, n, 65, dO.ptr, n, 0) != 0            # more than 64 columns
    assert f(hk.ctx, ctypes.byref(ok), 1, dB.ptr, n - 1, nc, dO.ptr, n, 0) != 0        # ldb < n
    assert f(hk.ctx, ctypes.byref(ok), 1, dB.ptr, n, nc, dO.ptr, n - 1, 0) != 0        # ldo < n
    assert f(hk.ctx, ctypes.byref(ok), 1, None, n, nc, dO.ptr, n, 0) != 0
    assert f(hk.ctx, ctypes.byref(ok), 1, dB.ptr, n, nc, None, n, 0) != 0
    assert f(hk.ctx, None, 1, dB.ptr, n, nc, dO.ptr, n, 0) != 0
    assert f(hk.ctx, ctypes.byref(ok), 2, dB.ptr, n, nc, dO.ptr, n, 0) != 0            # deriv is 0 or 1
    assert f(hk.ctx, ctypes.byref(ok), 1, dB.ptr, n, nc, dB.ptr, n, 0) != 0            # out aliases B
    assert f(hk.ctx, ctypes.byref(ok), 1, dB.ptr, n, nc, dO.ptr, n, -1) != 0
    # nothing to do
    assert f(hk.ctx, ctypes.byref(ok), 1, None, n, 0, None, n, 0) == 0
    assert f(hk.ctx, ctypes.byref(empty), 1, None, 0, nc, None, 0, 0) == 0
    hk.sync()
    assert np.array_equal(dO.get(), fill), "a refused call wrote its output"
    # more splits than stages: every split at least one stage
    B = rng.standard_normal((n, nc))
    X = dX.get().T
    a = matmul(hk, dX, n, d, 0, 1.3, 0.0, 1, B, 50)
    assert np.array_equal(a, matmul(hk, dX, n, d, 0, 1.3, 0.0, 1, B, 3))
    g, bp = g_reference(X, 0, 1.3, d, 1, 0.0)
    assert np.all(np.abs(a.astype(LD) - g @ B.astype(LD)) <= product_bound(g, bp, B))
    for v in (dX, dB, dO):
        v.free()


# ---- 3. hssk_coldots --------------------------------------------------------------------------------------------------------------
def check_coldots(hk, n, nc, seed=9):
    rng = np.random.default_rng(seed + n)
    lda, ldb = n + 2, n + 7
    A, B = np.full((lda, nc), 1e300), np.full((ldb, nc), 1e300)
    A[:n], B[:n] = rng.standard_normal((n, nc)), rng.standard_normal((n, nc))
    dA, dB, dO = hk.array(A), hk.array(B), hk.array(np.full(nc + 2, KC.SENTINEL))
    f = hk.lib.hssk_coldots
    hk.check(f(hk.ctx, dA.ptr, lda, dB.ptr, ldb, n, nc, dO.ptr))
    hk.sync()
    got = dO.get()
    assert np.all(got[nc:] == KC.SENTINEL)
    prod = A[:n].astype(LD) * B[:n].astype(LD)
    err, tol = np.abs(got[:nc].astype(LD) - prod.sum(0)), n * U * np.abs(prod).sum(0)
    print("coldots n=%d nc=%d: largest error / bound %.3f" % (n, nc, float((err / tol).max())))
    assert np.all(err <= tol), (n, nc)
    hk.check(f(hk.ctx, dA.ptr, lda, dB.ptr, ldb, n, nc, dO.ptr))
    hk.sync()
    assert np.array_equal(got, dO.get()), "two calls differ"
    assert f(hk.ctx, dA.ptr, n - 1, dB.ptr, ldb, n, nc, dO.ptr) != 0 and f(hk.ctx, None, lda, dB.ptr, ldb, n, nc, dO.ptr) != 0
    assert f(hk.ctx, dA.ptr, lda, dB.ptr, ldb, n, 0, None) == 0
    for v in (dA, dB, dO):
        v.free()


# ---- 4. the gradient of a kept model ----------------------------------------------------------------------------------------------
# The Gauss and Laplace rows of gp_cases.MODEL_CASES.
GRADIENT_CASES = [c for c in GP.MODEL_CASES if c[0] in KT]


def gradient_reference(kr, Hd, sv, kind, Z):
    """reference terms and their bounds (module docstring) for the probes Z (n x m, cluster order)"""
    ktype, _, h = kind
    X, alpha = kr.model_points(), kr.weights()
    n, d = X.shape
    g, bp = g_reference(X, ktype, h, d, 1, 0.0)
    W = bp + n * U * np.abs(g)
    cond = sv[0] / sv[-1]
    S = np.linalg.solve(Hd, Z)
    Gz = np.asarray(g @ Z.astype(LD), dtype=np.float64)
    E = np.asarray(W @ np.abs(Z).astype(LD), dtype=np.float64)
    F = np.linalg.norm
    th, tl = (S * Gz).sum(0), (S * Z).sum(0)
    bth = GP.EPS_F * cond * F(S, axis=0) * F(Gz, axis=0) + (np.abs(S) * E).sum(0)
    btl = GP.EPS_F * cond * F(S, axis=0) * F(Z, axis=0)
    al = alpha.astype(LD)
    quad_h, bqh = float(0.5 * (al @ (g @ al))), float(0.5 * (np.abs(al) @ (W @ np.abs(al))))
    quad_l = float(0.5 * (al @ al))
    ref = dict(th=th, tl=tl, quad_h=quad_h, quad_lambda=quad_l, trace_h=th.mean(), trace_lambda=tl.mean())
    bound = dict(th=bth, tl=btl, quad_h=bqh, quad_lambda=4 * U * quad_l, trace_h=bth.mean(), trace_lambda=btl.mean())
    ref["dh"], bound["dh"] = quad_h - 0.5 * ref["trace_h"], bqh + 0.5 * bound["trace_h"]
    ref["dlambda"], bound["dlambda"] = quad_l - 0.5 * ref["trace_lambda"], bound["quad_lambda"] + 0.5 * bound["trace_lambda"]
    return ref, bound


def check_gradient(kr, Hd, sv, kind, Z, tag, proves=True):
    """every term of the gradient with the probes Z under its bound, a second call bit for bit; returns (terms, worst ratio)"""
    ref, bound = gradient_reference(kr, Hd, sv, kind, Z)
    dh, dl, t = kr.log_marginal_likelihood_gradient(Z=Z, terms=True)
    t = dict(t, dh=dh, dlambda=dl)
    worst = 0.0
    for name in ("th", "tl", "quad_h", "quad_lambda", "trace_h", "trace_lambda", "dh", "dlambda"):
        err = np.abs(np.asarray(t[name]) - ref[name])
        ratio = float(np.max(err / bound[name]))
        worst = max(worst, ratio)
        print("gradient %s m=%d %s: reference %s largest error %.3g largest bound %.3g error / bound %.3g"
              % (tag, Z.shape[1], name, np.array2string(np.atleast_1d(ref[name])[:1], precision=9), float(np.max(err)),
                 float(np.max(bound[name])), ratio))
        assert np.all(err <= bound[name]), (tag, name, ratio)
    if proves:
        print("gradient %s: bound of dh %.3g, trace_h %.6g, quad_h %.6g" % (tag, bound["dh"], ref["trace_h"], ref["quad_h"]))
        assert bound["dh"] <= 1e-4 * min(abs(ref["trace_h"]), abs(ref["quad_h"])), (tag, bound["dh"], ref["trace_h"], ref["quad_h"])
    dh2, dl2, t2 = kr.log_marginal_likelihood_gradient(Z=Z, terms=True)
    assert (dh, dl) == (dh2, dl2) and all(np.array_equal(t[k], t2[k]) for k in t2), "two gradient calls differ"
    return t, worst


def rademacher(n, m, seed=23):
    return np.asfortranarray(np.random.default_rng(seed).choice([-1.0, 1.0], size=(n, m)))


def check_model_gradient(KM, lib, kern, d, lam, hscale, path):
    """one kept fit of gp_cases (n = 700): the gradient with 63 explicit Rademacher probes (one block with alpha)"""
    kr, _, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    tag = "%s R^%d lambda=%g h=%.3g" % (kern, d, lam, kind[2])
    try:
        Hd, sv, _ = GP.dense_model(kr, path)
        ld = kr.logabsdet()
        _, worst = check_gradient(kr, Hd, sv, kind, rademacher(kr.n, 63), tag)
        assert kr.logabsdet() == ld, "the gradient disturbed the kept model"
    finally:
        kr.destroy()
    return worst


# ---- 5. the exact trace, several blocks ---------------------------------------------------------------------------------------------
def check_exact_trace(KM, lib, path, n=192):
    """Gauss R^8, n = 192: the probes sqrt(n) e_k give the exact traces (three blocks of columns, alpha in the first only); and
    m = 1 (alpha and one probe), 64 (alpha pushes the last probe into a second block), 65 (a second block of two)"""
    kr, _, kind = GP.fit_model(KM, lib, "gauss", 8, 4.0, 1.0, n=n)
    try:
        Hd, sv, _ = GP.dense_model(kr, path)
        Z = np.asfortranarray(np.sqrt(n) * np.eye(n))
        t, _ = check_gradient(kr, Hd, sv, kind, Z, "exact trace n=%d" % n)
        ref, bound = gradient_reference(kr, Hd, sv, kind, Z)
        g, _ = g_reference(kr.model_points(), kind[0], kind[2], 8, 1, 0.0)
        trh = float(np.trace(np.linalg.solve(Hd, np.asarray(g, dtype=np.float64))))
        trl = float(np.trace(np.linalg.solve(Hd, np.eye(n))))
        print("exact trace: trace_h %.12g tr(Hd^-1 K') %.12g bound %.3g; trace_lambda %.12g tr(Hd^-1) %.12g bound %.3g"
              % (t["trace_h"], trh, bound["trace_h"], t["trace_lambda"], trl, bound["trace_lambda"]))
        # (the bound of a trace: the per-probe bounds summed and divided by the n probes)
        assert abs(t["trace_h"] - trh) <= bound["trace_h"] and abs(t["trace_lambda"] - trl) <= bound["trace_lambda"]
        for m in (1, 64, 65):
            check_gradient(kr, Hd, sv, kind, rademacher(n, m, 31 + m), "n=%d" % n, proves=False)
    finally:
        kr.destroy()


# ---- 6. the seeded form -------------------------------------------------------------------------------------------------------------
def check_seeded(KM, lib):
    kr, _, _ = GP.fit_model(KM, lib, "gauss", 8, 4.0, 1.0, n=192)
    try:
        Z7, Z8 = kr.model_probes(63, 7), kr.model_probes(63, 8)
        assert Z7.shape == (192, 63) and np.all(np.abs(Z7) == 1.0) and np.all(np.abs(Z8) == 1.0)
        assert not np.array_equal(Z7, Z8) and np.array_equal(Z7, kr.model_probes(63, 7))
        assert abs(Z7.mean()) < 0.05 and (Z7 == 1.0).any() and (Z7 == -1.0).any()
        a = kr.log_marginal_likelihood_gradient(probes=63, seed=7, terms=True)
        b = kr.log_marginal_likelihood_gradient(Z=Z7, terms=True)
        assert a[:2] == b[:2] and all(np.array_equal(a[2][k], b[2][k]) for k in a[2]), "seeded and explicit forms differ"
        c = kr.log_marginal_likelihood_gradient(probes=63, seed=8)
        assert c != a[:2]
        assert kr.log_marginal_likelihood_gradient() == kr.log_marginal_likelihood_gradient(probes=63, seed=0)
    finally:
        kr.destroy()


# ---- 7. the residual against the exact kernel matrix --------------------------------------------------------------------------------
def check_residual(kr, kind, tag, visible=True):
    """visible: the case asserts that its residual is far above its bound, so that it cannot pass on a zero"""
    ktype, _, h = kind
    X, y, alpha = kr.model_points(), kr.model_labels().astype(LD), kr.weights().astype(LD)
    n, d = X.shape
    g, bp = g_reference(X, ktype, h, d, 0, kr.lam)
    ref = float(np.sqrt(((y - g @ alpha) ** 2).sum() / (y ** 2).sum()))
    bound = float(np.sqrt((product_bound(g, bp, alpha[:, None]) ** 2).sum() / (y ** 2).sum()))
    got = kr.fit_residual()
    print("residual %s: got %.12g reference %.12g |error| %.3g bound %.3g" % (tag, got, ref, abs(got - ref), bound))
    assert not visible or ref >= 1e3 * bound, (tag, ref, bound)
    assert abs(got - ref) <= bound, (tag, got, ref, bound)
    assert got == kr.fit_residual()


def check_fit_residual(KM, lib, kern, d, lam, hscale):
    """a fit at the default (loose) compression tolerance of 1e-2"""
    kr, _, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    try:
        check_residual(kr, kind, "%s R^%d lambda=%g" % (kern, d, lam))
    finally:
        kr.destroy()


# ---- 8. after set_lambda ------------------------------------------------------------------------------------------------------------
def check_after_set_lambda(KM, lib, kern, d, lam1, lam2, hscale, path):
    kr, _, kind = GP.fit_model(KM, lib, kern, d, lam1, hscale)
    tag = "%s R^%d lambda %g -> %g" % (kern, d, lam1, lam2)
    try:
        Z = rademacher(kr.n, 63)
        g1 = kr.log_marginal_likelihood_gradient(Z=Z)
        kr.set_lambda(lam2)
        Hd, sv, _ = GP.dense_model(kr, path)
        check_gradient(kr, Hd, sv, kind, Z, tag)
        assert kr.log_marginal_likelihood_gradient(Z=Z) != g1
        # (a Laplace kernel matrix in R^1 is semiseparable: its compression is exact and its residual is rounding, 1e-15)
        check_residual(kr, kind, tag, visible=kern != "laplace" or d > 1)
    finally:
        kr.destroy()


# ---- 9. refusals and lifecycle ------------------------------------------------------------------------------------------------------
def gradient_calls(lib, Kh, n, m=3):
    """every new call on the raw handle with pre-filled outputs: [(name, return code, outputs untouched)]"""
    res = []
    grad, terms, Z = np.full(2, 123.25), np.full(4 + 2 * m, 123.25), np.ones((n, m), order="F")
    rc = lib.SPX_kernel_lml_gradient(Kh, m, Z.ctypes.data, 0, grad.ctypes.data, terms.ctypes.data)
    res.append(("lml_gradient(Z)", rc, bool(np.all(grad == 123.25) and np.all(terms == 123.25))))
    rc = lib.SPX_kernel_lml_gradient(Kh, m, None, 5, grad.ctypes.data, terms.ctypes.data)
    res.append(("lml_gradient(seed)", rc, bool(np.all(grad == 123.25) and np.all(terms == 123.25))))
    P = np.full((n, m), 123.25, order="F")
    res.append(("model_probes", lib.SPX_kernel_model_probes(Kh, m, 5, P.ctypes.data), bool(np.all(P == 123.25))))
    out = ctypes.c_double(123.25)
    res.append(("model_residual", lib.SPX_kernel_model_residual(Kh, ctypes.byref(out)), out.value == 123.25))
    return res


def check_gradient_lifecycle(KM, lib):
    n, d = 300, 8
    X, y, _ = GP.model_data(d, n, 20)
    h = float(KC.kernel_widths(d)[0])
    args = ["--hss_leaf_size", "64"]
    # no keep_model
    plain = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X, y)
    for name, rc, untouched in gradient_calls(lib, plain.K, n):
        assert rc != 0 and untouched, ("no keep_model", name, rc)
    for call in (plain.log_marginal_likelihood_gradient, plain.fit_residual, lambda: plain.model_probes(3, 1)):
        try:
            call()
            raise AssertionError("a handle without a kept model answered")
        except RuntimeError:
            pass
    plain.destroy()
    # a float handle
    kf = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X.astype(np.float32), y.astype(np.float32))
    for name, rc, untouched in gradient_calls(lib, kf.K, n):
        assert rc != 0 and untouched, ("float handle", name, rc)
    kf.destroy()
    # an ANOVA fit keeps a model, but has no derivative and no product
    ka = KM.KernelRegression(lib, h=h, lam=4.0, kernel="ANOVA", degree=2, argv=args, keep_model=True).fit(X, y)
    lda = ka.logabsdet()
    for name, rc, untouched in gradient_calls(lib, ka.K, n):
        if name != "model_probes":
            assert rc != 0 and untouched, ("ANOVA", name, rc)
    assert ka.logabsdet() == lda
    ka.destroy()
    # a kept Gauss model: m = 0, a wrong height, null outputs; the model answers as before afterwards
    kr = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X, y)
    ld, lml = kr.logabsdet(), kr.log_marginal_likelihood()
    grad, terms = np.full(2, 123.25), np.full(4, 123.25)
    assert lib.SPX_kernel_lml_gradient(kr.K, 0, None, 0, grad.ctypes.data, terms.ctypes.data) != 0
    assert lib.SPX_kernel_lml_gradient(kr.K, -1, None, 0, grad.ctypes.data, terms.ctypes.data) != 0
    assert lib.SPX_kernel_lml_gradient(kr.K, 3, None, 0, None, None) != 0
    assert lib.SPX_kernel_model_probes(kr.K, 0, 0, grad.ctypes.data) != 0
    assert np.all(grad == 123.25) and np.all(terms == 123.25)
    for bad in (np.ones((n - 1, 3)), np.ones((n + 1, 3)), np.ones((n, 0)), np.ones(n)):
        try:
            kr.log_marginal_likelihood_gradient(Z=bad)
            raise AssertionError("a probe block of shape %s was accepted" % (bad.shape,))
        except ValueError:
            pass
    try:
        kr.log_marginal_likelihood_gradient(probes=0)
        raise AssertionError("probes = 0 was accepted")
    except ValueError:
        pass
    for name, rc, untouched in gradient_calls(lib, kr.K, n):
        assert rc == 0 and not untouched, (name, rc)
    g1 = kr.log_marginal_likelihood_gradient(probes=5, seed=3)       # without the terms
    g2 = kr.log_marginal_likelihood_gradient(probes=5, seed=3, terms=True)
    assert g1 == g2[:2] and len(g2[2]["th"]) == 5 and np.all(np.isfinite(g2[2]["tl"]))
    assert kr.logabsdet() == ld and kr.log_marginal_likelihood() == lml, "the gradient disturbed the kept model"
    ms = kr.gradient_ms()
    assert set(ms) == {"product_ms", "solve_ms", "dots_ms"}
    # keep_model(false): the calls refuse again
    assert lib.SPX_kernel_keep_model(kr.K, 0) == 0
    for name, rc, untouched in gradient_calls(lib, kr.K, n):
        assert rc != 0 and untouched, ("after keep_model(false)", name, rc)
    kr.destroy()
