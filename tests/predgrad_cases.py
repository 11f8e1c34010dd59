"""Checks of the gradients of the predicted mean and variance in the test points (hssk_kernel_predict_grad,
Kernel<double>::predict_gradient / predict_variance_gradient / predict_variance_gradient_exact and their C and Python forms;
DESIGN.md 8j), shared by the CPU emulator tests (tests/test_predgrad_emu.py) and the GPU tests (tests/test_predgrad_gpu.py), as
tests/gp_cases.py is.

What is computed.  G(j, c) = sum_r w_rc dk(x_r, t_c) / dt_cj.  With delta_j = x_rj - t_cj the derivative of a pair is
    D_rjc = f delta_j              f = k / h^2 (Gauss), (3 / h^2) e^-s (Matern32), (5 / (3 h^2)) (1 + s) e^-s (Matern52)
    D_rjc = f sign(delta_j)        f = k / h (Laplace), sign(0) = 0
(d/dt of exp(-|x - t|^2 / (2 h^2)) is k (x - t) / h^2; of exp(-|x - t|_1 / h) it is k sign(x - t) / h; for the Matern kernels
dk/ds = -s e^-s and -s (1 + s) e^-s / 3 with ds/dt_j = -(2 nu / h^2) delta_j / s, so the s cancels and no form divides by the
distance).  The reference is long double numpy from the FP64 points: kernel_cases.kernel_ref for the types 0 and 1,
matern_cases.matern_ref for the types 3 and 4, and the differences x_rj - t_cj in long double.

The bound of one entry (u = 2^-53), counted from csrc/kernels/hssk_kpredict_grad.hip.
  k, s  the distance loop, the exponentials and s are those of hssk_kernel_predict: b_k = kernel_cases.kernel_entry_bound for Gauss
        and Laplace, a relative rho(d) u in s for the Matern kernels (matern_cases.rho).
  f     Gauss    exp(..) * (1 / (h h)): the product h h, the reciprocal, the product:    b_f = (b_k + 3 u k) / h^2
        Laplace  exp(..) * (1 / h): the reciprocal and the product:                       b_f = (b_k + 2 u k) / h
        Matern32 c e, c = 3 / (h h) (two roundings), e = exp(-s) within one unit in the last place (2 u) and moved by the error
                 of s (d ln f / d ln s = -s), the product:  5 u, taken as                  b_f = u f (rho(d) s + 6)
        Matern52 (c / 3) ((1 + s) e): c (2 u), c / 3, 1 + s, the exponential (2 u), two products, and |d ln f / d ln s| =
                 |s / (1 + s) - s| <= s:                                                  b_f = u f (rho(d) s + 8)
  term  phi = w f (one rounding), delta_j = x_rj - t_cj (one rounding, relative: a difference of FP64 inputs), phi delta_j (one
        rounding where the compiler does not fuse it into the addition): three are counted, four are allowed (second-order terms):
            term_rjc = |w_rc| (b_f |delta_j| + 4 u f |delta_j|).
        Laplace adds +-phi or 0: the sign of the computed difference is the sign of the true one, so |sign(delta_j)| (1 or 0)
        stands in the place of |delta_j|, and an agreeing coordinate contributes exactly nothing to the sum and to the bound.
  sum   the pairs of a split are added one after the other, then the split partials in split order:
            B_jc = sum_r term_rjc + (n + splits) u sum_r |w_rc f delta_j|.
A case only proves something while the entries themselves are large against their bounds: every kernel-level case asserts, for
every test column, max_j |G_jc| >= 1e3 max_j B_jc -- a statement about the reference alone.

The model.  gp_cases.fit_model / dense_model: Hd is the dense form of the written, compressed matrix, X the cluster-ordered points.
  mean      G_jc = sum_r alpha_r D_rjc with the handle's own weights, under sum_r |alpha_r| b_D,rjc + (n + s_max) u sum_r |alpha_r D_rjc|,
            b_D = b_f |delta_j| + 4 u f |delta_j| the term bound without its weight, s_max = ceil(n / 64) the largest split count
            the kernel can take (the automatic one depends on m; the issue's n u is this with the splits counted).
  variance  the reference is -2 D_c^T Hd^-1 k_c (module docstring of gp_cases.py with D_jc in the place of one k; the library forms
            z^ = Hd^-1 k^ + delta and adds z^_r D^_rjc):
                bound_jc = 2 [1e-12 cond_2 ||D_jc|| ||z_c|| + sum_r |z_rc| b_D,rjc + ||Hd^-1||_2 ||D_jc|| ||b_c||
                              + (n + s_max) u sum_r |z_rc D_rjc|],
            b_c the entry bounds of k_c.  Every case asserts bound <= 1e-3 of the column's largest reference component.
  exact     the same against the dense exact K + lambda I, plus the reported final relative residual times 2 cond ||D_jc|| ||k_c||.

Oracle validity (check_oracle, numpy only): the formulas above inside the dense mean and variance, against central differences in the
test point (step 1e-5, 1e-5 relative: the step and tolerance of matern_cases.check_oracle)."""
import ctypes

import numpy as np

import gp_cases as GP
import kernel_cases as KC
import matern_cases as MC
from strumpack_amd import hssk as K

LD = np.longdouble
U = KC.U53
S = KC.SENTINEL
TYPES = {"gauss": 0, "laplace": 1, "matern32": 3, "matern52": 4}
TILE = 64      # training points per stage of the kernel


def width(ktype, d):
    return float(KC.kernel_widths(d)[1 if ktype == 1 else 0])


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def factor_ref(X, T, ktype, h):
    """(f, b_f, k, b_k) in long double, n x m: the pair factor, its bound, the kernel value and its bound"""
    n, m, d = len(X), len(T), X.shape[1]
    Z = np.vstack([X, T])
    h = LD(h)
    if ktype in (0, 1):
        k, a, A = KC.kernel_ref(Z, np.arange(n), n + np.arange(m), ktype, h, 0.0)
        bk = KC.kernel_entry_bound(a, A, ktype, d, 0.0)
        if ktype == 0:
            return k / (h * h), (bk + 3 * U * k) / (h * h), k, bk
        return k / h, (bk + 2 * U * k) / h, k, bk
    k, s, dks, _ = MC.matern_ref(Z, np.arange(n), n + np.arange(m), ktype, h, 0.0)
    bk = MC.entry_bound(k, s, dks, d, 0.0)
    e = np.exp(-s)
    if ktype == 3:
        f = LD(3) / (h * h) * e
        return f, U * f * (MC.rho(d) * s + 6), k, bk
    f = LD(5) / (3 * h * h) * (1 + s) * e
    return f, U * f * (MC.rho(d) * s + 8), k, bk


def deriv_ref(X, T, ktype, h):
    """(D, b_D, k, b_k): D[r, j, c] = dk(x_r, t_c) / dt_cj in long double and the bound of one term without its weight"""
    f, bf, k, bk = factor_ref(X, T, ktype, h)
    delta = np.asarray(X, dtype=LD)[:, :, None] - np.asarray(T, dtype=LD).T[None, :, :]
    if ktype == 1:
        delta = np.sign(delta)
    D = f[:, None, :] * delta
    bD = (bf[:, None, :] + 4 * U * f[:, None, :]) * np.abs(delta)
    return D, bD, k, bk


def grad_ref(D, bD, W, splits):
    """(G, B), d x m, for the weights W (n x m) of the module docstring"""
    n = D.shape[0]
    Wl = np.asarray(W, dtype=LD)[:, None, :]
    G = (Wl * D).sum(0)
    B = (np.abs(Wl) * bD).sum(0) + (n + splits) * U * np.abs(Wl * D).sum(0)
    return G, B


# ---- oracle validity: the formulas against central differences of the dense mean and variance ----------------------------------------
def dense_kernel(A, Bp, ktype, h):
    return np.asarray(factor_ref(A, Bp, ktype, h)[2], dtype=np.float64)


def check_oracle(kern, d, n=200, lam=4.0, step=1e-5, m=3):
    ktype = TYPES[kern]
    h = width(ktype, d)
    X, y, T = GP.model_data(d, n, m + 2, 5)
    T = T[:m]                                                        # (none of them a training point)
    if ktype == 1:
        gap = np.abs(X[:, None, :] - T[None, :, :]).min()
        assert gap >= 10 * step, ("a test point within ten steps of a kink of the Laplace kernel", gap)
    Hm = dense_kernel(X, X, ktype, h) + lam * np.eye(n)              # symmetric: the formula is the derivative of the variance
    alpha = np.linalg.solve(Hm, y)

    def mean_var(P):
        kt = dense_kernel(X, P, ktype, h)
        return alpha @ kt, 1.0 - (kt * np.linalg.solve(Hm, kt)).sum(0)
    D = np.asarray(deriv_ref(X, T, ktype, h)[0], dtype=np.float64)
    z = np.linalg.solve(Hm, dense_kernel(X, T, ktype, h))
    gm = np.einsum("r,rjc->jc", alpha, D)
    gv = -2.0 * np.einsum("rc,rjc->jc", z, D)
    worst = 0.0
    for j in range(d):
        E = np.zeros((m, d))
        E[:, j] = step
        (mp, vp), (mm, vm) = mean_var(T + E), mean_var(T - E)
        fm, fv = (mp - mm) / (2 * step), (vp - vm) / (2 * step)
        em, ev = np.abs(gm[j] - fm) / np.abs(gm).max(0), np.abs(gv[j] - fv) / np.abs(gv).max(0)
        worst = max(worst, em.max(), ev.max())
    print("oracle %s R^%d: largest difference of d mean / dt and d var / dt from central differences, relative to the column's "
          "largest component: %.3g" % (kern, d, worst))
    assert worst <= 1e-5, (kern, d, worst)


# ---- hssk_kernel_predict_grad on its own ------------------------------------------------------------------------------------------------
# (n, m, d): one pair; around the four-wave coordinate split (3, 4, 5 coordinates) with 63, 64, 65 training / test points; more than
# one tile both ways; every count of coordinates per wave (2, 9, 16 of 16) and the largest dimension
GRAD_SHAPES = ((1, 1, 1), (63, 64, 3), (64, 65, 4), (65, 1, 5), (130, 130, 8), (257, 70, 33), (130, 65, 63), (70, 130, 64))


def grad_call(hk, spec, dW, ldw, dT, m, d, splits, ldg=None, extra=1):
    """one call into a pre-filled d x m block of leading dimension ldg with `extra` trailing columns: (G, whole block)"""
    ldg = d + 3 if ldg is None else ldg
    dG = hk.array(np.full((ldg, m + extra), S))
    hk.check(hk.lib.hssk_kernel_predict_grad(hk.ctx, ctypes.byref(spec), dW.ptr, ldw, dT.ptr, m, dG.ptr, ldg, splits))
    hk.sync()
    full = dG.get()
    dG.free()
    assert np.all(full[d:, :] == S) and np.all(full[:, m:] == S), "hssk_kernel_predict_grad wrote outside its block"
    return full[:d, :m], full


def split_counts(n):
    tiles = (n + TILE - 1) // TILE
    return sorted(set([1, 2, 3, tiles, tiles + 5]))


def check_predict_grad(hk, n, m, d, seed=11):
    """the four kernels, both weight modes, padded ldw and ldg, every split count: each entry under B_jc; the case proves something;
    two calls, the automatic and the forced count, equal weight columns and a column computed alone agree bit for bit"""
    rng = np.random.default_rng(seed + 7 * d + n)
    X, T = rng.standard_normal((n, d)), rng.standard_normal((m, d))
    if n >= 2 and m >= 2:
        T[-2:] = X[[min(3, n - 2), n - 1]]                     # the last two test points are training points
    W, w = rng.standard_normal((n, m)), rng.standard_normal(n)
    ldw = n + 5
    Wp = np.full((ldw, m), 1e300)
    Wp[:n] = W
    wcols = np.full((ldw, m), 1e300)
    wcols[:n] = w[:, None]
    dX, dT, dW, dw, dWw = hk.array(X.T), hk.array(T.T), hk.array(Wp), hk.array(w), hk.array(wcols)
    tiles = (n + TILE - 1) // TILE
    auto = hk.lib.hssk_kernel_predict_grad_splits(n, m)
    assert 1 <= auto <= tiles, (auto, tiles)
    worst = 0.0
    for name, ktype in TYPES.items():
        h = width(ktype, d)
        spec = K.KernelSpec(dX.ptr, n, d, ktype, 1, h, 2.0)       # (a lambda in the spec must not reach the gradient)
        D, bD, _, _ = deriv_ref(X, T, ktype, h)
        for mode, dev, ld, Wm in (("columns", dW, ldw, W), ("vector", dw, 0, np.tile(w[:, None], (1, m)))):
            got = {}
            for s in split_counts(n):
                eff = min(s, tiles)                               # (a request above the tile count is clamped)
                G, B = grad_ref(D, bD, Wm, eff)
                assert np.all(np.abs(G).max(0) >= 1e3 * B.max(0)), ("the case proves nothing", name, mode, n, m, d)
                got[s], _ = grad_call(hk, spec, dev, ld, dT, m, d, s)
                err = np.abs(got[s].astype(LD) - G)
                frac = float((err / np.where(B > 0, B, 1)).max())
                assert np.all(err <= B), (name, mode, n, m, d, s, frac)
                worst = max(worst, frac)
            assert np.array_equal(got[tiles], got[tiles + 5]), "a split count above the tile count is not the tile count"
            again, _ = grad_call(hk, spec, dev, ld, dT, m, d, 2, ldg=d, extra=0)      # (unpadded: one reduction launch)
            assert np.array_equal(again, got[2]), "two calls differ"
            a0, _ = grad_call(hk, spec, dev, ld, dT, m, d, 0)
            assert np.array_equal(a0, got[auto] if auto in got else grad_call(hk, spec, dev, ld, dT, m, d, auto)[0]), "splits = 0"
            if mode == "vector":
                eq, _ = grad_call(hk, spec, dWw, ldw, dT, m, d, 2)
                assert np.array_equal(eq, got[2]), "equal weight columns differ from the single vector"
            # one test point alone: its column does not depend on m, on the other points or on its position
            c = m // 2
            dT1 = hk.array(T[c:c + 1].T)
            dW1 = hk.array(Wp[:, c:c + 1]) if mode == "columns" else dw
            one, _ = grad_call(hk, spec, dW1, ld, dT1, 1, d, 2)
            assert np.array_equal(one[:, 0], got[2][:, c]), (name, mode, "a column computed alone differs")
            dT1.free()
            if mode == "columns":
                dW1.free()
        print("kernel_predict_grad %s n=%d m=%d d=%d: largest error / bound %.3f" % (name, n, m, d, worst))
    for v in (dX, dT, dW, dw, dWw):
        v.free()
    return worst


def check_exact_zeros(hk, d=5):
    """n = 1: a test point equal to the training point gives G == 0 for the four kernels; a Laplace pair that agrees in one
    coordinate gives exactly 0 in that coordinate (and not in the others)"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, d))
    t = np.vstack([x, x + rng.standard_normal((1, d))])
    t[1, 2] = x[0, 2]
    dX, dT, dw = hk.array(x.T), hk.array(t.T), hk.array(np.array([1.7]))
    for name, ktype in TYPES.items():
        spec = K.KernelSpec(dX.ptr, 1, d, ktype, 1, width(ktype, d), 0.0)
        G, _ = grad_call(hk, spec, dw, 0, dT, 2, d, 0)
        assert np.all(G[:, 0] == 0.0), (name, G[:, 0])
        assert G[2, 1] == 0.0 and np.all(np.delete(G[:, 1], 2) != 0.0), (name, G[:, 1])
    for v in (dX, dT, dw):
        v.free()


def check_grad_refusals(hk):
    """nothing to do, the empty sum, and every refusal with its pre-filled output unchanged"""
    n, m, d = 70, 5, 4
    rng = np.random.default_rng(5)
    dX, dT, dW = hk.array(rng.standard_normal((d, n))), hk.array(rng.standard_normal((d, m))), hk.array(rng.standard_normal((n, m)))
    L, ctx = hk.lib, hk.ctx
    fill = np.full((d + 1, m + 1), S)
    dG = hk.array(fill)

    def call(spec, W, ldw, T, mm, G, ldg, splits, c=ctx):
        rc = L.hssk_kernel_predict_grad(c, ctypes.byref(spec) if spec is not None else None, W, ldw, T, mm, G, ldg, splits)
        hk.sync()
        return rc
    ok = K.KernelSpec(dX.ptr, n, d, 0, 1, 1.0, 0.0)
    assert call(ok, dW.ptr, n, dT.ptr, 0, None, d + 1, 0) == 0                    # m == 0: nothing to do
    assert np.array_equal(dG.get(), fill)
    refused = [
        ("no context", 1, lambda: call(ok, dW.ptr, n, dT.ptr, m, dG.ptr, d + 1, 0, c=None)),
        ("no kernel", 1, lambda: call(None, dW.ptr, n, dT.ptr, m, dG.ptr, d + 1, 0)),
        ("no weights", 1, lambda: call(ok, None, n, dT.ptr, m, dG.ptr, d + 1, 0)),
        ("no test points", 1, lambda: call(ok, dW.ptr, n, None, m, dG.ptr, d + 1, 0)),
        ("no points", 1, lambda: call(K.KernelSpec(None, n, d, 0, 1, 1.0, 0.0), dW.ptr, n, dT.ptr, m, dG.ptr, d + 1, 0)),
        ("m < 0", 1, lambda: call(ok, dW.ptr, n, dT.ptr, -1, dG.ptr, d + 1, 0)),
        ("ldg < d", 1, lambda: call(ok, dW.ptr, n, dT.ptr, m, dG.ptr, d - 1, 0)),
        ("0 < ldw < n", 1, lambda: call(ok, dW.ptr, n - 1, dT.ptr, m, dG.ptr, d + 1, 0)),
        ("ldw < 0", 1, lambda: call(ok, dW.ptr, -1, dT.ptr, m, dG.ptr, d + 1, 0)),
        ("splits < 0", 1, lambda: call(ok, dW.ptr, n, dT.ptr, m, dG.ptr, d + 1, -1)),
        ("type 5", 1, lambda: call(K.KernelSpec(dX.ptr, n, d, 5, 1, 1.0, 0.0), dW.ptr, n, dT.ptr, m, dG.ptr, d + 1, 0)),
        ("type -1", 1, lambda: call(K.KernelSpec(dX.ptr, n, d, -1, 1, 1.0, 0.0), dW.ptr, n, dT.ptr, m, dG.ptr, d + 1, 0)),
        ("ANOVA", 2, lambda: call(K.KernelSpec(dX.ptr, n, d, 2, 2, 1.0, 0.0), dW.ptr, n, dT.ptr, m, dG.ptr, d + 1, 0)),
        ("d > 64", 2, lambda: call(K.KernelSpec(dX.ptr, 4, 65, 0, 1, 1.0, 0.0), dW.ptr, 4, dT.ptr, 1, dG.ptr, 66, 0)),
    ]
    for what, code, f in refused:
        assert f() == code, what
        assert np.array_equal(dG.get(), fill), (what, "a refused call wrote")
    assert call(ok, None, n, dT.ptr, m, None, d + 1, 0) == 1 and np.array_equal(dG.get(), fill)        # no output
    # n == 0: the empty sum, inside the block only
    empty = K.KernelSpec(None, 0, d, 1, 1, 1.0, 0.0)
    assert call(empty, None, 0, dT.ptr, m, dG.ptr, d + 1, 0) == 0
    z = dG.get()
    assert np.all(z[:d, :m] == 0.0) and np.all(z[d:, :] == S) and np.all(z[:, m:] == S)
    for v in (dX, dT, dW, dG):
        v.free()


# ---- the kept model -------------------------------------------------------------------------------------------------------------------
# Gauss and Laplace in R^1, R^8 and R^64 at the (lambda, factor on the width) pairs of gp_cases.MODEL_CASES whose variance case
# proves something (R^64 takes the pairs of R^70 there)
MODEL_CASES = ([("gauss", 1, 4.0, 0.25), ("gauss", 1, 16.0, 1.0), ("gauss", 8, 4.0, 1.0), ("gauss", 8, 0.05, 0.5),
                ("gauss", 64, 4.0, 1.0), ("gauss", 64, 0.05, 1.0)]
               + [("laplace", d, lam, 1.0) for d in (1, 8, 64) for lam in (4.0, 0.05)])
COUNTS_CASE = ("gauss", 8, 4.0, 1.0)          # also answers for 1, 64 and 65 test points: a chunk, a full one, a full one and a rest


def s_max(n):
    return (n + TILE - 1) // TILE


def mean_reference(kr, T, kind, ref=None):
    """ref: deriv_ref of the model's points and T, where the caller has it already"""
    ktype, _, h = kind
    X, alpha = kr.model_points(), kr.weights()
    n = len(X)
    D, bD, _, _ = ref if ref is not None else deriv_ref(X, T, ktype, h)
    al = alpha.astype(LD)[:, None, None]
    G = (al * D).sum(0)
    B = (np.abs(al) * bD).sum(0) + (n + s_max(n)) * U * np.abs(al * D).sum(0)
    return G, B


def check_mean_gradient(kr, T, kind, tag, ref=None):
    G, B = mean_reference(kr, T, kind, ref)
    got = kr.predict_gradient(T)
    assert got.shape == T.shape
    err = np.abs(got.T.astype(LD) - G)
    ratio = float((err / B).max())
    print("mean gradient %s m=%d: largest component %.3g, largest bound %.3g, largest error / bound %.3g"
          % (tag, len(T), float(np.abs(G).max()), float(B.max()), ratio))
    assert np.all(np.abs(G).max(0) >= 1e3 * B.max(0)), (tag, "the case proves nothing")
    assert np.all(err <= B), (tag, ratio)
    assert np.array_equal(got, kr.predict_gradient(T)), "two gradient calls differ"
    return ratio


def variance_reference(Hm, sv, X, T, kind, ref=None):
    """(-2 D^T Hm^-1 k, bound) of the module docstring, d x m, for the dense matrix Hm with singular values sv"""
    ktype, _, h = kind
    n = len(X)
    D, bD, k, bk = ref if ref is not None else deriv_ref(X, T, ktype, h)
    D, bD, k, bk = (np.asarray(v, dtype=np.float64) for v in (D, bD, k, bk))
    z = np.linalg.solve(Hm, k)
    ref = -2.0 * np.einsum("rc,rjc->jc", z, D)
    cond, inv = sv[0] / sv[-1], 1.0 / sv[-1]
    nD = np.linalg.norm(D, axis=0)
    bound = 2.0 * (GP.EPS_F * cond * nD * np.linalg.norm(z, axis=0)[None, :] + np.einsum("rc,rjc->jc", np.abs(z), bD)
                   + inv * nD * np.linalg.norm(bk, axis=0)[None, :] + (n + s_max(n)) * U * np.einsum("rc,rjc->jc", np.abs(z), np.abs(D)))
    return ref, bound, nD, np.linalg.norm(k, axis=0)


def check_variance_gradient(kr, Hd, sv, T, kind, tag, ref=None):
    ref, bound, _, _ = variance_reference(Hd, sv, kr.model_points(), T, kind, ref)
    var, got = kr.predict_variance_gradient(T)
    assert got.shape == T.shape
    err = np.abs(got.T - ref)
    ratio = float((err / bound).max())
    print("variance gradient %s m=%d: largest component %.3g, largest bound %.3g, largest error %.3g, largest error / bound %.3g"
          % (tag, len(T), np.abs(ref).max(), bound.max(), err.max(), ratio))
    assert np.all(bound.max(0) <= 1e-3 * np.abs(ref).max(0)), (tag, "the case proves nothing", float((bound.max(0) / np.abs(ref).max(0)).max()))
    assert np.all(err <= bound), (tag, ratio)
    assert np.array_equal(var, kr.predict_variance(T)), "the variances next to the gradient are not those of predict_variance"
    v2, g2 = kr.predict_variance_gradient(T)
    assert np.array_equal(var, v2) and np.array_equal(got, g2), "two calls differ"
    return ratio


def check_model(KM, lib, kern, d, lam, hscale, path):
    """one fit with keep_model: both gradients of the 130 test points (chunks of 64, 64 and 2) against the dense form of the kept
    matrix; the COUNTS_CASE also for 1, 64 and 65 test points"""
    kr, T, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    tag = "%s R^%d lambda=%g h=%.3g" % (kern, d, lam, kind[2])
    try:
        Hd, sv, _ = GP.dense_model(kr, path)
        worst = 0.0
        for m in (130,) + ((1, 64, 65) if (kern, d, lam, hscale) == COUNTS_CASE else ()):
            ref = deriv_ref(kr.model_points(), T[-m:], kind[0], kind[2])          # (computed once for both gradients)
            worst = max(worst, check_mean_gradient(kr, T[-m:], kind, tag, ref), check_variance_gradient(kr, Hd, sv, T[-m:], kind, tag, ref))
    finally:
        kr.destroy()
    return worst


def check_exact(KM, lib, kern="gauss", d=8, lam=4.0, hscale=1.0, m=66):
    """exact=True against the dense exact K + lambda I: the bound with that matrix, plus the reported final relative residual
    times 2 cond ||D_jc|| ||k_c||; the variances are those of predict_variance(exact=True); inner="f32" returns, with the
    variances of predict_variance(exact=True, inner="f32")"""
    kr, T, kind = GP.fit_model(KM, lib, kern, d, lam, hscale)
    T = T[-m:]
    try:
        X = kr.model_points()
        Km = dense_kernel(X, X, kind[0], kind[2]) + lam * np.eye(len(X))
        sv = np.linalg.svd(Km, compute_uv=False)
        ref, bound, nD, nk = variance_reference(Km, sv, X, T, kind)
        var, got, info = kr.predict_variance_gradient(T, exact=True, info=True)
        assert info["converged"], info
        tol = bound + info["residual"][None, :] * 2.0 * (sv[0] / sv[-1]) * nD * nk[None, :]
        err = np.abs(got.T - ref)
        ratio = float((err / tol).max())
        print("exact variance gradient %s R^%d: largest component %.3g, largest tolerance %.3g, largest error / tolerance %.3g, %d steps"
              % (kern, d, np.abs(ref).max(), tol.max(), ratio, info["iterations"]))
        assert np.all(bound.max(0) <= 1e-3 * np.abs(ref).max(0)), "the case proves nothing"
        assert np.all(err <= tol), ratio
        assert np.array_equal(var, kr.predict_variance(T, exact=True))
        v32, g32 = kr.predict_variance_gradient(T, exact=True, inner="f32")
        assert np.all(np.isfinite(g32)) and g32.shape == T.shape
        assert np.array_equal(v32, kr.predict_variance(T, exact=True, inner="f32"))
        assert kr.krylov_inner()[0] == "f64"                       # (the mode of one call does not stay)
    finally:
        kr.destroy()
    return ratio


def check_widths(KM, lib, kern="gauss", d=8, lam=4.0):
    """a fit with widths = w: the gradient is that of the plain fit on X / w at T / w, divided by w, within the bound (the two run
    the same arithmetic on the same scaled points: in fact bit for bit), and that gradient is within the bound of its reference"""
    X, y, T = GP.model_data(d)
    ktype, p = GP.KINDS[kern]
    h = width(ktype, d)
    w = np.linspace(0.5, 2.0, d)
    a = KM.KernelRegression(lib, h=h, lam=lam, kernel=GP.KERNEL_NAMES[kern], argv=GP.FIT_ARGS, keep_model=True, widths=w).fit(X, y)
    b = KM.KernelRegression(lib, h=h, lam=lam, kernel=GP.KERNEL_NAMES[kern], argv=GP.FIT_ARGS, keep_model=True).fit(X / w, y)
    try:
        ga, gb = a.predict_gradient(T), b.predict_gradient(T / w) / w
        G, B = mean_reference(b, T / w, (ktype, p, h))
        assert np.all(np.abs(ga.T.astype(LD) - gb.T.astype(LD)) <= B / w[:, None])
        assert np.all(np.abs(ga.T.astype(LD) - G / w[:, None]) <= B / w[:, None] + U * np.abs(G / w[:, None]))   # (the division rounds once)
        va, gva = a.predict_variance_gradient(T)
        vb, gvb = b.predict_variance_gradient(T / w)
        assert np.array_equal(va, vb) and np.array_equal(gva, gvb / w)
    finally:
        a.destroy()
        b.destroy()


def check_refusals(KM, lib):
    """a float fit, an ANOVA fit, a fit without keep_model (the variance calls only), 65 coordinates, a handle before its fit: each
    refuses with the outputs untouched"""
    n, d, m = 300, 8, 5
    X, y, T = GP.model_data(d, n, m)
    T = np.ascontiguousarray(T)
    h = float(KC.kernel_widths(d)[0])
    args = ["--hss_leaf_size", "64"]

    def raw(Kh, Tp, dd):
        """[(name, return code, outputs untouched)] of the three C calls"""
        res = []
        g, v = np.full((len(Tp), dd), S), np.full(len(Tp), S)
        res.append(("mean", lib.SPX_kernel_predict_gradient_double(Kh, len(Tp), Tp.ctypes.data, g.ctypes.data), bool(np.all(g == S))))
        g = np.full((len(Tp), dd), S)
        res.append(("variance", lib.SPX_kernel_predict_variance_gradient_double(Kh, len(Tp), Tp.ctypes.data, v.ctypes.data, g.ctypes.data),
                    bool(np.all(g == S) and np.all(v == S))))
        g, v = np.full((len(Tp), dd), S), np.full(len(Tp), S)
        res.append(("exact", lib.SPX_kernel_predict_variance_gradient_exact_double(Kh, len(Tp), Tp.ctypes.data, v.ctypes.data, g.ctypes.data,
                                                                                  1e-8, 100, 30, None), bool(np.all(g == S) and np.all(v == S))))
        return res

    def raises(f):
        try:
            f()
        except (RuntimeError, ValueError):
            return True
        return False
    kf = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X.astype(np.float32), y.astype(np.float32))
    for name, rc, untouched in raw(kf.K, T, d):
        assert rc != 0 and untouched, ("float handle", name, rc)
    assert raises(lambda: kf.predict_gradient(T)) and raises(lambda: kf.predict_variance_gradient(T))
    kf.destroy()
    ka = KM.KernelRegression(lib, h=h, lam=4.0, kernel="ANOVA", degree=2, argv=args, keep_model=True).fit(X, y)
    for name, rc, untouched in raw(ka.K, T, d):
        assert rc != 0 and untouched, ("ANOVA", name, rc)
    assert raises(lambda: ka.predict_gradient(T)) and raises(lambda: ka.predict_variance_gradient(T))
    ka.destroy()
    kp = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args).fit(X, y)           # no kept model: the mean gradient works
    res = raw(kp.K, T, d)
    assert res[0][1] == 0 and not res[0][2], res[0]
    for name, rc, untouched in res[1:]:
        assert rc != 0 and untouched, ("no kept model", name, rc)
    assert kp.predict_gradient(T).shape == (m, d) and raises(lambda: kp.predict_variance_gradient(T))
    assert raises(lambda: kp.predict_variance_gradient(T, exact=True))
    kp.destroy()
    X65, y65, T65 = GP.model_data(65, n, m)
    T65 = np.ascontiguousarray(T65)
    k65 = KM.KernelRegression(lib, h=float(KC.kernel_widths(65)[0]), lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X65, y65)
    for name, rc, untouched in raw(k65.K, T65, 65):
        assert rc != 0 and untouched, ("65 coordinates", name, rc)
    assert raises(lambda: k65.predict_gradient(T65)) and raises(lambda: k65.predict_variance_gradient(T65))
    k65.destroy()
    # before the first fit; and the argument checks of the exact call on a fitted handle
    Xc = np.ascontiguousarray(X)
    Kh = lib.STRUMPACK_create_kernel_double(n, d, Xc.ctypes.data, h, 4.0, 1, 0)
    assert Kh and lib.SPX_kernel_keep_model(Kh, 1) == 0
    for name, rc, untouched in raw(Kh, T, d):
        assert rc != 0 and untouched, ("before the fit", name, rc)
    lib.STRUMPACK_destroy_kernel_double(Kh)
    kk = KM.KernelRegression(lib, h=h, lam=4.0, kernel="rbf", argv=args, keep_model=True).fit(X, y)
    g, v = np.full((m, d), S), np.full(m, S)
    for rtol, maxit, restart in ((0.0, 100, 30), (float("nan"), 100, 30), (1e-8, 0, 30), (1e-8, 100, 0)):
        assert lib.SPX_kernel_predict_variance_gradient_exact_double(kk.K, m, T.ctypes.data, v.ctypes.data, g.ctypes.data, rtol, maxit, restart, None) != 0
        assert np.all(g == S) and np.all(v == S)
    assert lib.SPX_kernel_predict_gradient_double(kk.K, -1, T.ctypes.data, g.ctypes.data) != 0
    assert lib.SPX_kernel_predict_gradient_double(kk.K, m, None, g.ctypes.data) != 0 and np.all(g == S)
    assert kk.predict_gradient(T[:0]).shape == (0, d)
    v0, g0 = kk.predict_variance_gradient(T[:0])
    assert v0.shape == (0,) and g0.shape == (0, d)
    kk.destroy()
