"""ctypes binding of the kernel ridge regression C interface (include/kernel/Kernel.h), the same entry points the
reference's src/python/STRUMPACKKernel.py.in binds: STRUMPACK_create_kernel_double / _kernel_fit_HSS_double /
_kernel_predict_double / _destroy_kernel_double."""
import ctypes as C

import numpy as np

KERNEL_SYMBOLS = [
    "STRUMPACK_create_kernel_double", "STRUMPACK_destroy_kernel_double", "STRUMPACK_kernel_fit_HSS_double",
    "STRUMPACK_kernel_predict_double", "SPX_kernel_fit_info", "SPX_kernel_permutation", "SPX_kernel_weights",
    "SPX_clustering", "SPX_clustering_device", "SPX_kernel_node_info", "SPX_kernel_set_neighbors", "SPX_approximate_neighbors",
    "STRUMPACK_create_kernel_float", "STRUMPACK_destroy_kernel_float", "STRUMPACK_kernel_fit_HSS_float",
    "STRUMPACK_kernel_predict_float", "SPX_kernel_predict_device_float", "SPX_kernel_predict_stats",
    "SPX_kernel_keep_model", "SPX_kernel_logabsdet", "SPX_kernel_log_marginal_likelihood", "SPX_kernel_predict_variance_double",
    "SPX_kernel_variance_ms", "SPX_kernel_model_set_lambda", "SPX_kernel_model_write", "SPX_kernel_model_labels",
    "SPX_kernel_model_points", "SPX_kernel_lml_gradient", "SPX_kernel_lml_gradient_coords", "SPX_kernel_model_probes", "SPX_kernel_model_residual",
    "SPX_kernel_gradient_ms", "SPX_kernel_model_refine", "SPX_kernel_model_solve", "SPX_kernel_predict_variance_exact_double",
    "SPX_kernel_krylov_ms", "SPX_kernel_set_krylov_inner", "SPX_kernel_krylov_inner", "SPX_kernel_krylov_stats",
    "SPX_kernel_predict_gradient_double", "SPX_kernel_predict_variance_gradient_double",
    "SPX_kernel_predict_variance_gradient_exact_double",
    "SPX_kernel_predict_covariance_double", "SPX_kernel_predict_covariance_exact_double", "SPX_kernel_covariance_ms",
]
KRYLOV_INNER = {"f64": 0, "f32": 1}
KERNEL_TYPES = {"Gauss": 0, "rbf": 0, "Laplace": 1, "ANOVA": 2}
CLUSTERING = {"natural": 0, "2means": 1, "kdtree": 2, "pca": 3, "cobble": 4}


def load(path):
    import torch  # noqa: F401  (first: its bundled HIP runtime must be the one in the process)
    L = C.CDLL(path)
    vp = C.c_void_p
    L.STRUMPACK_create_kernel_double.restype = vp
    L.STRUMPACK_create_kernel_double.argtypes = [C.c_int, C.c_int, vp, C.c_double, C.c_double, C.c_int, C.c_int]
    L.STRUMPACK_destroy_kernel_double.argtypes = [vp]
    L.STRUMPACK_kernel_fit_HSS_double.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_char_p)]
    L.STRUMPACK_kernel_predict_double.argtypes = [vp, C.c_int, vp, vp]
    L.STRUMPACK_create_kernel_float.restype = vp
    L.STRUMPACK_create_kernel_float.argtypes = [C.c_int, C.c_int, vp, C.c_float, C.c_float, C.c_int, C.c_int]
    L.STRUMPACK_destroy_kernel_float.argtypes = [vp]
    L.STRUMPACK_kernel_fit_HSS_float.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_char_p)]
    L.STRUMPACK_kernel_predict_float.argtypes = [vp, C.c_int, vp, vp]
    L.SPX_kernel_predict_device_float.argtypes = [vp, C.c_int, vp, vp]
    L.SPX_kernel_predict_stats.argtypes = [vp, vp]
    L.SPX_kernel_fit_info.argtypes = [vp, vp]
    L.SPX_kernel_permutation.argtypes = [vp, vp]
    L.SPX_kernel_weights.argtypes = [vp, vp]
    L.SPX_kernel_node_info.argtypes = [vp, vp, C.c_int]
    L.SPX_kernel_set_neighbors.argtypes = [vp, C.c_int, vp]
    L.SPX_approximate_neighbors.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp]
    L.SPX_kernel_keep_model.argtypes = [vp, C.c_int]
    L.SPX_kernel_logabsdet.argtypes = [vp, C.POINTER(C.c_double)]
    L.SPX_kernel_log_marginal_likelihood.argtypes = [vp, C.POINTER(C.c_double)]
    L.SPX_kernel_predict_variance_double.argtypes = [vp, C.c_int, vp, vp]
    L.SPX_kernel_variance_ms.argtypes = [vp, vp]
    L.SPX_kernel_model_set_lambda.argtypes = [vp, C.c_double]
    L.SPX_kernel_model_write.argtypes = [vp, C.c_char_p]
    L.SPX_kernel_model_labels.argtypes = [vp, vp]
    L.SPX_kernel_model_points.argtypes = [vp, vp]
    L.SPX_kernel_lml_gradient.argtypes = [vp, C.c_int, vp, C.c_ulonglong, vp, vp]
    L.SPX_kernel_lml_gradient_coords.argtypes = [vp, C.c_int, vp, C.c_ulonglong, vp, vp]
    L.SPX_kernel_model_probes.argtypes = [vp, C.c_int, C.c_ulonglong, vp]
    L.SPX_kernel_model_residual.argtypes = [vp, C.POINTER(C.c_double)]
    L.SPX_kernel_gradient_ms.argtypes = [vp, vp]
    L.SPX_kernel_model_refine.argtypes = [vp, C.c_double, C.c_int, C.c_int, vp]
    L.SPX_kernel_model_solve.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_double, C.c_int, C.c_int, vp]
    L.SPX_kernel_predict_variance_exact_double.argtypes = [vp, C.c_int, vp, vp, C.c_double, C.c_int, C.c_int, vp]
    L.SPX_kernel_predict_gradient_double.argtypes = [vp, C.c_int, vp, vp]
    L.SPX_kernel_predict_variance_gradient_double.argtypes = [vp, C.c_int, vp, vp, vp]
    L.SPX_kernel_predict_variance_gradient_exact_double.argtypes = [vp, C.c_int, vp, vp, vp, C.c_double, C.c_int, C.c_int, vp]
    L.SPX_kernel_predict_covariance_double.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    L.SPX_kernel_predict_covariance_exact_double.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_double, C.c_int, C.c_int, vp]
    L.SPX_kernel_covariance_ms.argtypes = [vp, vp]
    L.SPX_kernel_krylov_ms.argtypes = [vp, vp]
    L.SPX_kernel_set_krylov_inner.argtypes = [vp, C.c_int, C.c_double]
    L.SPX_kernel_krylov_inner.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.SPX_kernel_krylov_stats.argtypes = [vp, vp]
    L.SPX_clustering.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int]
    L.SPX_clustering_device.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp]
    return L


class KernelRegression:
    """Kernel ridge regression classifier, same shape as the reference's STRUMPACKKernel (fit / predict)."""

    def __init__(self, lib, h=1.0, lam=4.0, kernel="rbf", degree=1, argv=(), keep_model=False, widths=None):
        """keep_model (double fits only): the fit keeps its factored matrix, so that logabsdet, log_marginal_likelihood,
        predict_variance, set_lambda and write_model work afterwards.  widths (None, or d positive values): one length scale per
        coordinate (automatic relevance determination), k(x / widths, y / widths): fit divides the columns of X by them, and so
        do decision_function, predict and predict_variance with their test points; the model then holds the scaled points.
        None changes nothing anywhere."""
        self.L, self.h, self.lam, self.ktype, self.p, self.argv = lib, h, lam, KERNEL_TYPES[kernel], degree, list(argv)
        self.K, self.dtype, self.keep_model = None, np.dtype(np.float64), bool(keep_model)
        self.widths = None
        if widths is not None:
            w = np.array(widths, dtype=np.float64)
            if w.ndim != 1 or w.size < 1 or not np.all(np.isfinite(w)) or not np.all(w > 0.0):
                raise ValueError("widths: a vector of positive, finite length scales, one per coordinate")
            self.widths = w

    def _scaled(self, P, what):
        """the points P (rows) in the coordinates the model works in: divided by widths where those are set"""
        if self.widths is None:
            return P
        if P.ndim != 2 or P.shape[1] != len(self.widths):
            raise ValueError("%s: %d widths, but points with shape %s" % (what, len(self.widths), P.shape))
        return P / self.widths.astype(P.dtype)

    def fit(self, X, y, neighbors=None):
        """float32 X: the float entry points (promoted fit, FP32 prediction; the fit works on a copy of X, kept in cluster
        order as self.X_); any other dtype: the double ones"""
        self.destroy()
        self.dtype = np.dtype(np.float32 if np.asarray(X).dtype == np.float32 else np.float64)
        sfx = "float" if self.dtype == np.float32 else "double"
        X = np.array(X, dtype=self.dtype, order="C")     # n x d row-major == d x n column-major
        X = np.ascontiguousarray(self._scaled(X, "fit"))
        y = np.array(y, dtype=self.dtype, order="C")
        self.n, self.d = X.shape
        self.X_, self.y_ = X, y   # (the float entry points reorder both in place and keep pointing at X)
        self.K = getattr(self.L, "STRUMPACK_create_kernel_" + sfx)(self.n, self.d, X.ctypes.data, self.h, self.lam, self.p, self.ktype)
        if not self.K:
            raise RuntimeError("STRUMPACK_create_kernel_%s failed" % sfx)
        if neighbors is not None:   # tests: k x n lists in cluster order (see include/kernel/Kernel.h)
            nb = np.ascontiguousarray(neighbors, dtype=np.int32)
            self.L.SPX_kernel_set_neighbors(self.K, nb.shape[1], nb.ctypes.data)
        if self.keep_model and self.L.SPX_kernel_keep_model(self.K, 1):
            raise RuntimeError("SPX_kernel_keep_model failed (a double fit with a built-in kernel is needed)")
        args = [b"kernel"] + [a.encode() for a in self.argv]
        argv = (C.c_char_p * len(args))(*args)
        getattr(self.L, "STRUMPACK_kernel_fit_HSS_" + sfx)(self.K, y.ctypes.data, len(args), argv)
        return self

    # ---- the kept model (keep_model=True) ----
    def logabsdet(self):
        """log|det H| of the compressed K + lambda I"""
        out = C.c_double(0.0)
        if self.L.SPX_kernel_logabsdet(self.K, C.byref(out)):
            raise RuntimeError("SPX_kernel_logabsdet failed (no kept model)")
        return out.value

    def log_marginal_likelihood(self):
        out = C.c_double(0.0)
        if self.L.SPX_kernel_log_marginal_likelihood(self.K, C.byref(out)):
            raise RuntimeError("SPX_kernel_log_marginal_likelihood failed (no kept model)")
        return out.value

    def predict_variance(self, T, exact=False, rtol=1e-8, maxit=100, restart=30, info=False, inner=None, inner_rtol=None):
        """variance of the latent function at the rows of T (add lam for the observation noise); not clamped: the compressed
        matrix is K + lam I only up to the compression tolerance, so a value may be slightly negative.  exact=True: the solve
        with the exact kernel matrix instead (see refine), up to rtol; info=True then also returns the dict of that solve;
        inner / inner_rtol: see refine"""
        T = np.ascontiguousarray(self._scaled(np.asarray(T, dtype=np.float64), "predict_variance"))
        out = np.zeros(T.shape[0])
        if not exact:
            if self.L.SPX_kernel_predict_variance_double(self.K, T.shape[0], T.ctypes.data, out.ctypes.data):
                raise RuntimeError("SPX_kernel_predict_variance_double failed (no kept model)")
            return out
        buf = np.zeros(8 + 2 * T.shape[0])
        with self._inner(inner, inner_rtol):
            if self.L.SPX_kernel_predict_variance_exact_double(self.K, T.shape[0], T.ctypes.data, out.ctypes.data, float(rtol), int(maxit),
                                                               int(restart), buf.ctypes.data):
                raise RuntimeError("SPX_kernel_predict_variance_exact_double failed (a kept model of a Gauss or Laplace fit and valid "
                                   "rtol / maxit / restart are needed; inner=\"f32\": at most 64 coordinates)")
            return (out, self._krylov_stats(self._krylov_info(buf))) if info else out

    # ---- gradients in the test points (double fits, Gauss and Laplace, at most 64 coordinates) ----
    def _unscaled_gradient(self, G):
        """a gradient in the model's coordinates t / widths in the caller's: the chain rule divides by widths"""
        return G if self.widths is None else G / self.widths

    def predict_gradient(self, T):
        """(m, d): the gradient of decision_function in the rows of T, sum_r alpha_r dk(x_r, t) / dt -- a force, where the fit is an
        energy surface.  With widths set the result is in the caller's coordinates.  No kept model needed."""
        if self.dtype == np.float32:
            raise RuntimeError("predict_gradient: a double fit is needed")
        T = np.ascontiguousarray(self._scaled(np.asarray(T, dtype=np.float64), "predict_gradient"))
        if T.ndim != 2 or T.shape[1] != self.d:
            raise ValueError("predict_gradient: an m x d array of test points is expected")
        G = np.zeros((T.shape[0], self.d))
        if self.L.SPX_kernel_predict_gradient_double(self.K, T.shape[0], T.ctypes.data, G.ctypes.data):
            raise RuntimeError("SPX_kernel_predict_gradient_double failed (a double Gauss or Laplace fit in at most 64 coordinates is needed)")
        return self._unscaled_gradient(G)

    def predict_variance_gradient(self, T, exact=False, rtol=1e-8, maxit=100, restart=30, info=False, inner=None, inner_rtol=None):
        """(var, grad[, info]): predict_variance(T, ...) -- the same values, bit for bit -- and its gradient in the rows of T, (m, d):
        -2 sum_r V_r dk(x_r, t) / dt with V = H^-1 k(X, t) (exact=True: the exact solve).  This is the derivative of the returned
        variance exactly when the kept matrix is symmetric; otherwise it is -2 D^T H^-1 k.  With widths set the gradient is in
        the caller's coordinates.  The other arguments: see predict_variance."""
        if self.dtype == np.float32:
            raise RuntimeError("predict_variance_gradient: a double fit is needed")
        T = np.ascontiguousarray(self._scaled(np.asarray(T, dtype=np.float64), "predict_variance_gradient"))
        if T.ndim != 2 or T.shape[1] != self.d:
            raise ValueError("predict_variance_gradient: an m x d array of test points is expected")
        m = T.shape[0]
        var, G = np.zeros(m), np.zeros((m, self.d))
        if not exact:
            if self.L.SPX_kernel_predict_variance_gradient_double(self.K, m, T.ctypes.data, var.ctypes.data, G.ctypes.data):
                raise RuntimeError("SPX_kernel_predict_variance_gradient_double failed (a kept model of a Gauss or Laplace fit in at most "
                                   "64 coordinates is needed)")
            return var, self._unscaled_gradient(G)
        buf = np.zeros(8 + 2 * m)
        with self._inner(inner, inner_rtol):
            if self.L.SPX_kernel_predict_variance_gradient_exact_double(self.K, m, T.ctypes.data, var.ctypes.data, G.ctypes.data, float(rtol),
                                                                        int(maxit), int(restart), buf.ctypes.data):
                raise RuntimeError("SPX_kernel_predict_variance_gradient_exact_double failed (a kept model of a Gauss or Laplace fit in at "
                                   "most 64 coordinates and valid rtol / maxit / restart are needed)")
            G = self._unscaled_gradient(G)
            return (var, G, self._krylov_stats(self._krylov_info(buf))) if info else (var, G)

    # ---- the joint predictive covariance and draws from it (double fits, Gauss and Laplace) ----
    def predict_covariance(self, T, exact=False, rtol=1e-8, maxit=100, restart=30, info=False, inner=None, inner_rtol=None):
        """(m, m): the joint covariance of the latent function at the rows of T, k(T, T) - (Q + Q^T) / 2 with
        Q = k(T, X) H^-1 k(X, T); exactly symmetric, not clamped (a loosely compressed fit can give an indefinite matrix).  Its
        diagonal agrees with predict_variance(T) within rounding, not bit for bit: the sums run in another order.  With widths set
        the rows of T are scaled like everywhere else; the covariance needs no scaling back.  The other arguments: see
        predict_variance."""
        if self.dtype == np.float32:
            raise RuntimeError("predict_covariance: a double fit is needed")
        T = np.ascontiguousarray(self._scaled(np.asarray(T, dtype=np.float64), "predict_covariance"))
        if T.ndim != 2 or T.shape[1] != self.d:
            raise ValueError("predict_covariance: an m x d array of test points is expected")
        m = T.shape[0]
        cov = np.zeros((m, m), order="F")
        if not exact:
            if self.L.SPX_kernel_predict_covariance_double(self.K, m, T.ctypes.data, cov.ctypes.data, m):
                raise RuntimeError("SPX_kernel_predict_covariance_double failed (a kept model of a Gauss or Laplace fit is needed)")
            return cov
        buf = np.zeros(8 + 2 * m)
        with self._inner(inner, inner_rtol):
            if self.L.SPX_kernel_predict_covariance_exact_double(self.K, m, T.ctypes.data, cov.ctypes.data, m, float(rtol), int(maxit),
                                                                 int(restart), buf.ctypes.data):
                raise RuntimeError("SPX_kernel_predict_covariance_exact_double failed (a kept model of a Gauss or Laplace fit and valid "
                                   "rtol / maxit / restart are needed; inner=\"f32\": at most 64 coordinates)")
            return (cov, self._krylov_stats(self._krylov_info(buf))) if info else cov

    def covariance_ms(self):
        out = np.zeros(3)
        if self.L.SPX_kernel_covariance_ms(self.K, out.ctypes.data):
            raise RuntimeError("no kept double-precision Gauss or Laplace model")
        return dict(zip(["cross_ms", "solve_ms", "product_ms"], out.tolist()))

    def sample_posterior(self, T, nsamples, seed=0, exact=False, jitter=0.0, **krylov):
        """(nsamples, m): joint draws of the LATENT function at the rows of T, mean + Z L^T with mean = decision_function(T) (for a
        classification fit: the latent value, not its sign), Z = Generator(Philox(seed)).standard_normal((nsamples, m)) and
        L = cholesky(predict_covariance(T, exact, **krylov) + jitter I).  Raises ValueError where that matrix is not positive
        definite (a covariance from a loosely compressed fit can be indefinite)."""
        C_ = self.predict_covariance(T, exact=exact, **krylov)
        m = C_.shape[0]
        A = C_ + float(jitter) * np.eye(m)
        try:
            Lc = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            raise ValueError("sample_posterior: covariance + jitter I is not positive definite (smallest eigenvalue %.3e); use "
                             "exact=True or a larger jitter" % (np.linalg.eigvalsh(A).min() if m else 0.0)) from None
        Z = np.random.Generator(np.random.Philox(int(seed))).standard_normal((int(nsamples), m))
        return np.asarray(self.decision_function(T), dtype=np.float64).reshape(1, m) + Z @ Lc.T

    # ---- the precision of the product inside the cycles of refine / solve / predict_variance(exact=True) ----
    def set_krylov_inner(self, inner="f64", inner_rtol=None):
        """handle state, like keep_model: "f64" (the default) or "f32" -- the FP32 matrix-core product inside the restart cycles,
        FP64 true residuals at their starts; inner_rtol in (0, 1) (None: the library's default, 1e-4): a column leaves its cycle at
        max(rtol ||b||, inner_rtol ||r at the cycle's start||)"""
        if inner not in KRYLOV_INNER:
            raise ValueError('inner must be "f64" or "f32"')
        if inner_rtol is not None and not 0.0 < float(inner_rtol) < 1.0:      # (also not-a-number)
            raise RuntimeError("inner_rtol must lie in (0, 1)")
        if self.L.SPX_kernel_set_krylov_inner(self.K, KRYLOV_INNER[inner], 0.0 if inner_rtol is None else float(inner_rtol)):
            raise RuntimeError("SPX_kernel_set_krylov_inner failed (a double handle with a built-in kernel is needed)")
        return self

    def krylov_inner(self):
        """(inner, inner_rtol) as set"""
        p, r = C.c_int(0), C.c_double(0.0)
        if self.L.SPX_kernel_krylov_inner(self.K, C.byref(p), C.byref(r)):
            raise RuntimeError("SPX_kernel_krylov_inner failed (a double handle with a built-in kernel is needed)")
        return ("f32" if p.value else "f64"), r.value

    def _inner(self, inner, inner_rtol):
        """context: the mode of one call.  inner=None: the handle's own mode (set_krylov_inner; "f64" unless set); "f64" / "f32"
        force that precision for this call whatever the handle says; inner_rtol=None: the handle's.  The handle's mode is
        restored afterwards."""
        kr = self

        class Mode:
            def __enter__(self):
                self.old = None
                if inner is not None or inner_rtol is not None:
                    self.old = kr.krylov_inner()
                    kr.set_krylov_inner(self.old[0] if inner is None else inner, self.old[1] if inner_rtol is None else inner_rtol)

            def __exit__(self, *exc):
                if self.old is not None:
                    kr.set_krylov_inner(*self.old)
                return False
        return Mode()

    def _krylov_stats(self, d):
        """the counts of the last call that the 8 + 2 m info doubles have no room for"""
        st = np.zeros(6)
        if self.L.SPX_kernel_krylov_stats(self.K, st.ctypes.data) == 0:
            d["products32"], d["fallbacks"] = int(st[1]), int(st[2])
        return d

    @staticmethod
    def _krylov_info(buf):
        m = int(buf[7])
        return dict(converged=bool(buf[0]), iterations=int(buf[1]), products=int(buf[2]), solves=int(buf[3]), cycles=int(buf[4]),
                    residual0=float(buf[5]), residual_max=float(buf[6]), residual=buf[8:8 + m].copy(),
                    its=buf[8 + m:8 + 2 * m].astype(np.int64), products32=0, fallbacks=0)

    def refine(self, rtol=1e-8, maxit=100, restart=30, inner=None, inner_rtol=None):
        """weights of the EXACT K + lam I: restarted GMRES on the device with the kept factors as preconditioner, from the
        current weights.  weights(), decision_function, fit_residual and log_marginal_likelihood follow; logabsdet stays that of
        the compressed matrix.  Returns a dict: converged, iterations, products, solves, cycles, residual0 (before), residual
        (after; both true relative residuals), its, products32, fallbacks.  Not converging within maxit steps is reported, not
        raised.  inner=None runs in the handle's mode (set_krylov_inner; FP64 unless set), "f64" and "f32" force the precision of
        this call.  inner="f32": the product inside the cycles is the FP32
        matrix-core one, `products` counts the FP64 products alone (one per cycle start), `products32` the others, `fallbacks`
        the blocks that went back to FP64 because a true residual did not decrease; inner_rtol: see set_krylov_inner."""
        buf = np.zeros(10)
        with self._inner(inner, inner_rtol):
            if self.L.SPX_kernel_model_refine(self.K, float(rtol), int(maxit), int(restart), buf.ctypes.data):
                raise RuntimeError("SPX_kernel_model_refine failed (a kept model of a Gauss or Laplace fit and valid rtol / maxit / restart "
                                   "are needed; inner=\"f32\": at most 64 coordinates)")
        d = self._krylov_stats(self._krylov_info(buf))
        d["residual"] = float(d["residual"][0])
        d["its"] = int(d["its"][0])
        del d["residual_max"]
        return d

    def solve(self, B, rtol=1e-8, maxit=100, restart=30, inner=None, inner_rtol=None):
        """(X, dict) with (K + lam I) X = B for the exact kernel matrix; B: n or n x m, rows in cluster order (the order of
        model_points()).  The model is not changed.  residual and its of the dict are per column."""
        B = np.asarray(B, dtype=np.float64)
        one = B.ndim == 1
        B = np.asfortranarray(B.reshape(len(B), -1))
        if B.shape[0] != self.n:
            raise ValueError("solve: B must have n rows")
        m = B.shape[1]
        X, buf = np.zeros((self.n, m), order="F"), np.zeros(8 + 2 * m)
        with self._inner(inner, inner_rtol):
            if self.L.SPX_kernel_model_solve(self.K, m, B.ctypes.data, self.n, X.ctypes.data, self.n, float(rtol), int(maxit), int(restart),
                                             buf.ctypes.data):
                raise RuntimeError("SPX_kernel_model_solve failed (a kept model of a Gauss or Laplace fit and valid rtol / maxit / restart "
                                   "are needed; inner=\"f32\": at most 64 coordinates)")
        return (X[:, 0] if one else X), self._krylov_stats(self._krylov_info(buf))

    def krylov_ms(self):
        out = np.zeros(3)
        if self.L.SPX_kernel_krylov_ms(self.K, out.ctypes.data):
            raise RuntimeError("no kept double-precision Gauss or Laplace model")
        return dict(zip(["product_ms", "solve_ms", "krylov_ms"], out.tolist()))

    def variance_ms(self):
        out = np.zeros(3)
        if self.L.SPX_kernel_variance_ms(self.K, out.ctypes.data):
            raise RuntimeError("no kept model")
        return dict(zip(["cross_ms", "solve_ms", "colsum_ms"], out.tolist()))

    def set_lambda(self, lam):
        """a new lambda on the kept compression: shift, factor, solve; weights() and the predictions follow"""
        if self.L.SPX_kernel_model_set_lambda(self.K, float(lam)):
            raise RuntimeError("SPX_kernel_model_set_lambda failed (no kept model)")
        self.lam = float(lam)
        return self

    def write_model(self, path):
        if self.L.SPX_kernel_model_write(self.K, str(path).encode()):
            raise RuntimeError("SPX_kernel_model_write failed (no kept model)")

    def model_labels(self):
        y = np.zeros(self.n)
        if self.L.SPX_kernel_model_labels(self.K, y.ctypes.data):
            raise RuntimeError("no kept model")
        return y

    def model_points(self):
        """the training points in cluster order (n x d) as the model holds them: with widths set, the SCALED points X / widths"""
        X = np.zeros((self.n, self.d))
        if self.L.SPX_kernel_model_points(self.K, X.ctypes.data):
            raise RuntimeError("no kept model")
        return X

    def model_probes(self, m, seed=0):
        """the n x m block of +-1 probes the seeded gradient uses (rows in cluster order)"""
        Z = np.zeros((self.n, int(m)), order="F")
        if self.L.SPX_kernel_model_probes(self.K, int(m), int(seed), Z.ctypes.data):
            raise RuntimeError("SPX_kernel_model_probes failed (no kept model, or m < 1)")
        return Z

    def log_marginal_likelihood_gradient(self, probes=63, seed=0, Z=None, terms=False):
        """(dL/dh, dL/dlambda) of the log marginal likelihood: the exact kernel derivative against the kept, compressed inverse,
        the traces estimated with `probes` Rademacher vectors from `seed`, or with the columns of Z (n x m, rows in cluster order:
        the order of model_points()).  terms=True: also a dict with quad_h, quad_lambda, trace_h, trace_lambda and the per-probe
        values th, tl (their spread gives the standard error of the trace estimates)."""
        if Z is not None:
            Z = np.asfortranarray(Z, dtype=np.float64)
            if Z.ndim != 2 or Z.shape[0] != self.n or Z.shape[1] < 1:
                raise ValueError("log_marginal_likelihood_gradient: Z must be n x m with m >= 1")
            m, zp = Z.shape[1], Z.ctypes.data
        else:
            m, zp = int(probes), None
        if m < 1:
            raise ValueError("log_marginal_likelihood_gradient: at least one probe vector")
        grad, t = np.zeros(2), np.zeros(4 + 2 * m)
        if self.L.SPX_kernel_lml_gradient(self.K, m, zp, int(seed), grad.ctypes.data, t.ctypes.data):
            raise RuntimeError("SPX_kernel_lml_gradient failed (a kept model of a Gauss or Laplace fit is needed)")
        if not terms:
            return float(grad[0]), float(grad[1])
        return float(grad[0]), float(grad[1]), dict(quad_h=t[0], quad_lambda=t[1], trace_h=t[2], trace_lambda=t[3],
                                                    th=t[4:4 + m].copy(), tl=t[4 + m:].copy())

    def log_marginal_likelihood_gradient_coords(self, probes=63, seed=0, Z=None, terms=False):
        """the gradient of the log marginal likelihood in one length scale per coordinate (Gauss and Laplace, d <= 64): a length-d
        array.  With widths set: dL/dwidths_j of the kernel k(x / widths, y / widths).  Without: dL/dtheta_j, theta_j = ln l_j
        at l = 1 (the same number as dL/dwidths at widths = 1); its sum over j is h dL/dh.  The exact matrices K o D_j against the
        kept, compressed inverse; probes, seed and Z as in log_marginal_likelihood_gradient.  terms=True: also a dict with dtheta,
        quad and trace (length d) and the per-probe values tc (d x m)."""
        if Z is not None:
            Z = np.asfortranarray(Z, dtype=np.float64)
            if Z.ndim != 2 or Z.shape[0] != self.n or Z.shape[1] < 1:
                raise ValueError("log_marginal_likelihood_gradient_coords: Z must be n x m with m >= 1")
            m, zp = Z.shape[1], Z.ctypes.data
        else:
            m, zp = int(probes), None
        if m < 1:
            raise ValueError("log_marginal_likelihood_gradient_coords: at least one probe vector")
        d = self.d
        grad, t = np.zeros(d), np.zeros(2 * d + d * m)
        if self.L.SPX_kernel_lml_gradient_coords(self.K, m, zp, int(seed), grad.ctypes.data, t.ctypes.data):
            raise RuntimeError("SPX_kernel_lml_gradient_coords failed (a kept model of a Gauss or Laplace fit in at most 64 "
                               "coordinates is needed)")
        out = grad.copy() if self.widths is None else grad / self.widths
        if not terms:
            return out
        return out, dict(dtheta=grad, quad=t[:d].copy(), trace=t[d:2 * d].copy(), tc=t[2 * d:].reshape(d, m).copy())

    def gradient_ms(self):
        out = np.zeros(3)
        if self.L.SPX_kernel_gradient_ms(self.K, out.ctypes.data):
            raise RuntimeError("no kept model")
        return dict(zip(["product_ms", "solve_ms", "dots_ms"], out.tolist()))

    def fit_residual(self):
        """||y - (K + lam I) alpha|| / ||y|| with the EXACT kernel matrix: how far the compressed fit is from the exact one"""
        out = C.c_double(0.0)
        if self.L.SPX_kernel_model_residual(self.K, C.byref(out)):
            raise RuntimeError("SPX_kernel_model_residual failed (a kept model of a Gauss or Laplace fit is needed)")
        return out.value

    def decision_function(self, T):
        """T: m x d array; after a float32 fit also a float32 torch tensor on the device (m x d, contiguous), which is
        read in place and answered by a tensor on the same device"""
        if self.dtype == np.float32 and type(T).__module__.startswith("torch") and T.is_cuda:
            import torch
            if T.dtype != torch.float32 or not T.is_contiguous() or T.dim() != 2 or T.shape[1] != self.d:
                raise ValueError("decision_function: a contiguous float32 m x d tensor is expected")
            if self.widths is not None:
                T = (T / torch.as_tensor(self.widths, dtype=torch.float32, device=T.device)).contiguous()
            out = torch.empty(T.shape[0], dtype=torch.float32, device=T.device)
            torch.cuda.synchronize(T.device)
            if self.L.SPX_kernel_predict_device_float(self.K, T.shape[0], T.data_ptr(), out.data_ptr()):
                raise RuntimeError("SPX_kernel_predict_device_float failed")
            return out
        T = np.ascontiguousarray(self._scaled(np.asarray(T, dtype=self.dtype), "decision_function"))
        out = np.zeros(T.shape[0], dtype=self.dtype)
        sfx = "float" if self.dtype == np.float32 else "double"
        getattr(self.L, "STRUMPACK_kernel_predict_" + sfx)(self.K, T.shape[0], T.ctypes.data, out.ctypes.data)
        return out

    def predict_stats(self):
        out = np.zeros(6, dtype=np.int64)
        if self.L.SPX_kernel_predict_stats(self.K, out.ctypes.data):
            raise RuntimeError("no float prediction")
        return dict(zip(["mfma_tiles", "diff_tiles", "splits", "device_us", "uploaded_bytes", "resident"], out.tolist()))

    def predict(self, T):
        return np.where(self.decision_function(T) >= 0, 1.0, -1.0)

    def info(self):
        out = np.zeros(8, dtype=np.int64)
        if self.L.SPX_kernel_fit_info(self.K, out.ctypes.data):
            raise RuntimeError("no fit")
        return dict(zip(["compressed", "levels", "rank", "memory", "neighbors", "compress_us", "factor_us", "solve_us"], out.tolist()))

    def node_info(self):
        out = np.zeros((1 << 16, 6), dtype=np.int32)
        c = self.L.SPX_kernel_node_info(self.K, out.ctypes.data, 1 << 16)
        return out[:c].copy()

    def permutation(self):
        p = np.zeros(self.n, dtype=np.int32)
        self.L.SPX_kernel_permutation(self.K, p.ctypes.data)
        return p

    def weights(self):
        w = np.zeros(self.n)
        if self.L.SPX_kernel_weights(self.K, w.ctypes.data):
            raise RuntimeError("no fit")
        return w.astype(self.dtype)   # (a float handle hands out its float weights widened: narrowing them is exact)

    def destroy(self):
        if getattr(self, "K", None):
            getattr(self.L, "STRUMPACK_destroy_kernel_" + ("float" if self.dtype == np.float32 else "double"))(self.K)
            self.K = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def clustering(lib, X, algo="2means", leaf_size=512):
    """binary_tree_clustering on its own: returns (reordered points, 1-based permutation, leaf sizes)."""
    X = np.ascontiguousarray(X, dtype=np.float64).copy()
    n, d = X.shape
    perm = np.zeros(n, dtype=np.int32)
    ls = np.zeros(max(16, 4 * n // max(leaf_size, 1) + 16), dtype=np.int32)
    c = lib.SPX_clustering(n, d, X.ctypes.data, CLUSTERING[algo], leaf_size, perm.ctypes.data, ls.ctypes.data, len(ls))
    if c < 0:
        raise RuntimeError("SPX_clustering failed")
    return X, perm, ls[:c].copy()


def clustering_device(lib, X, algo="cobble", leaf_size=512):
    """The median-split partitioners on the device (SPX_clustering_device): returns (status, reordered points, 1-based
    permutation, leaf sizes); status != 0: the device form stood back (ties, long displacement chains) and nothing was moved."""
    X = np.ascontiguousarray(X, dtype=np.float64).copy()
    n, d = X.shape
    perm = np.zeros(n, dtype=np.int32)
    ls = np.zeros(max(16, 4 * n // max(leaf_size, 1) + 16), dtype=np.int32)
    st = C.c_int(0)
    c = lib.SPX_clustering_device(n, d, X.ctypes.data, CLUSTERING[algo], leaf_size, perm.ctypes.data, ls.ctypes.data, len(ls), C.byref(st))
    if c < 0:
        raise RuntimeError("SPX_clustering_device failed")
    return st.value, X, perm, ls[:c].copy()


def approximate_neighbors(lib, X, k, iterations=5):
    """find_approximate_neighbors (the reference's randomized projection-tree search, host): returns ids (n x k)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, d = X.shape
    out = np.zeros((n, k), dtype=np.int32)
    if lib.SPX_approximate_neighbors(n, d, X.ctypes.data, iterations, k, out.ctypes.data, None):
        raise RuntimeError("SPX_approximate_neighbors failed")
    return out
