"""Timing of the gradient kernel hssk_kernel_predict_grad against the prediction kernels of the same shape, in one process on one GPU:

  * kernel lines: N training points uniform in [0, 1)^8, Gauss and Laplace, h = 1.3; the single-vector mode at m = 64, 1e4 and 1e5
    against hssk_kernel_predict, and the column mode at m = 64 (the shape of a variance chunk) against hssk_kernel_predict_cols.
    Device-clock stopwatches (hssk_watch_*) around each call, two warm-up calls, then --reps calls: minimum, median, maximum.
    The two kernels of a shape alternate inside the timed loop.
  * with --model: a kept Gauss fit of the same points, then predict_variance and predict_variance_gradient of 64 test points by the
    host clock (both end in a device-to-host copy), with the device-clock parts of SPX_kernel_variance_ms: the cost of one
    variance-gradient chunk next to the variance chunk itself.
  * with --sweep: the single-vector Gauss call at m = 64, 1e3 and 1e4 with forced split counts around the automatic one (what the
    constant behind hssk_kernel_predict_grad_splits was chosen from).

  python tools/predict_grad_bench.py [--n 100000] [--reps 7] [--model | --sweep]

Prints one JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from strumpack_amd import _loader  # noqa: E402
from strumpack_amd import hssk as K  # noqa: E402
from strumpack_amd import kernel as KM  # noqa: E402

H, D = 1.3, 8
KINDS = (("gauss", 0), ("laplace", 1))


def stats(ms):
    return dict(ms_min=round(min(ms), 4), ms_median=round(float(np.median(ms)), 4), ms_max=round(max(ms), 4))


def kernel_lines(hk, n, reps, sizes):
    lib = hk.lib
    lib.hssk_watch_start.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_stop.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_read_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.hssk_watch_read_ms.restype = C.c_double
    r = np.random.default_rng(2025)
    X, w = r.random((n, D)), r.standard_normal(n)
    dX, dw = hk.array(X.ravel()), hk.array(w)

    def timed(calls):
        """calls: name -> function; every round runs each once (alternating), two rounds of warm-up"""
        ms = {k: [] for k in calls}
        for it in range(reps + 2):
            for k, f in calls.items():
                hk.check(lib.hssk_watch_start(hk.ctx, 0))
                hk.check(f())
                hk.check(lib.hssk_watch_stop(hk.ctx, 0))
                v = lib.hssk_watch_read_ms(hk.ctx, 0, None)
                if it >= 2:
                    ms[k].append(v)
        return ms
    for m in sizes:
        T = r.random((m, D))
        dT, dP, dG = hk.array(T.ravel()), hk.empty((m,)), hk.empty((D, m))
        dW = hk.array(r.standard_normal((n, m))) if m <= 64 else None
        for name, kt in KINDS:
            spec = K.KernelSpec(dX.ptr, n, D, kt, 1, H, 0.0)
            modes = [("vector", lambda: lib.hssk_kernel_predict(hk.ctx, C.byref(spec), dw.ptr, dT.ptr, m, dP.ptr),
                      lambda: lib.hssk_kernel_predict_grad(hk.ctx, C.byref(spec), dw.ptr, 0, dT.ptr, m, dG.ptr, D, 0))]
            if dW is not None:
                modes.append(("columns", lambda: lib.hssk_kernel_predict_cols(hk.ctx, C.byref(spec), dW.ptr, n, dT.ptr, m, dP.ptr),
                              lambda: lib.hssk_kernel_predict_grad(hk.ctx, C.byref(spec), dW.ptr, n, dT.ptr, m, dG.ptr, D, 0)))
            for mode, value, grad in modes:
                ms = timed({"value": value, "gradient": grad})
                hk.sync()
                g = dG.get()
                assert np.all(np.isfinite(g))
                print(json.dumps(dict(what="predict_grad_kernel", kernel=name, mode=mode, n=n, m=m, d=D, reps=reps,
                                      splits=int(lib.hssk_kernel_predict_grad_splits(n, m)),
                                      value=stats(ms["value"]), gradient=stats(ms["gradient"]),
                                      gradient_over_value=round(min(ms["gradient"]) / min(ms["value"]), 4),
                                      gpairs_per_s=round(float(n) * m / (min(ms["gradient"]) * 1e-3) * 1e-9, 2))), flush=True)
        for a in (dT, dP, dG) + ((dW,) if dW is not None else ()):
            a.free()
    dX.free()
    dw.free()


def sweep_lines(hk, n, reps):
    lib = hk.lib
    lib.hssk_watch_start.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_stop.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_read_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.hssk_watch_read_ms.restype = C.c_double
    r = np.random.default_rng(2025)
    dX, dw = hk.array(r.random((n, D)).ravel()), hk.array(r.standard_normal(n))
    spec = K.KernelSpec(dX.ptr, n, D, 0, 1, H, 0.0)
    stages = (n + 63) // 64
    for m in (64, 1000, 10000):
        dT, dG = hk.array(r.random((m, D)).ravel()), hk.empty((D, m))
        tiles, auto = (m + 63) // 64, int(lib.hssk_kernel_predict_grad_splits(n, m))
        out = {}
        for wgs in (128, 256, 512, 768, 1024, 1536, 2048, 4096):
            s = max(1, min(stages, -(-wgs // tiles)))
            if s in out:
                continue
            ms = []
            for it in range(reps + 2):
                hk.check(lib.hssk_watch_start(hk.ctx, 0))
                hk.check(lib.hssk_kernel_predict_grad(hk.ctx, C.byref(spec), dw.ptr, 0, dT.ptr, m, dG.ptr, D, s))
                hk.check(lib.hssk_watch_stop(hk.ctx, 0))
                v = lib.hssk_watch_read_ms(hk.ctx, 0, None)
                if it >= 2:
                    ms.append(v)
            out[s] = dict(workgroups=s * tiles, **stats(ms))
        print(json.dumps(dict(what="predict_grad_split_sweep", kernel="gauss", n=n, m=m, d=D, reps=reps, automatic=auto, splits=out)), flush=True)
        dT.free()
        dG.free()
    dX.free()
    dw.free()


def model_lines(n, reps):
    lib = KM.load(_loader.lib_path())
    r = np.random.default_rng(2025)
    X = r.random((n, D))
    y = np.sign((X - 0.5) @ r.standard_normal(D))
    T = r.random((64, D))
    argv = ["--hss_leaf_size", "128", "--hss_rel_tol", "1e-2", "--hss_abs_tol", "1e-8", "--hss_approximate_neighbors", "64"]
    kr = KM.KernelRegression(lib, h=H, lam=3.11, kernel="rbf", argv=argv, keep_model=True).fit(X, y)
    wall = {"variance": [], "variance_gradient": []}
    parts = None
    for it in range(reps + 2):
        t0 = time.perf_counter()
        v = kr.predict_variance(T)
        t1 = time.perf_counter()
        parts = kr.variance_ms()
        t2 = time.perf_counter()
        v2, g = kr.predict_variance_gradient(T)
        t3 = time.perf_counter()
        assert np.array_equal(v, v2) and np.all(np.isfinite(g))
        if it >= 2:
            wall["variance"].append((t1 - t0) * 1e3)
            wall["variance_gradient"].append((t3 - t2) * 1e3)
    t0 = time.perf_counter()
    gm = kr.predict_gradient(T)
    mean_ms = (time.perf_counter() - t0) * 1e3
    assert np.all(np.isfinite(gm))
    print(json.dumps(dict(what="variance_gradient_chunk", n=n, m=64, d=D, reps=reps, variance=stats(wall["variance"]),
                          variance_gradient=stats(wall["variance_gradient"]), variance_device_parts_ms=parts,
                          extra_ms=round(min(wall["variance_gradient"]) - min(wall["variance"]), 4),
                          predict_gradient_host_ms=round(mean_ms, 3))), flush=True)
    kr.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="64,10000,100000")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    if a.model:
        model_lines(a.n, max(a.reps, 3))
        return
    hk = K.Hssk(_loader.lib_path())
    if a.sweep:
        sweep_lines(hk, a.n, max(a.reps, 3))
        hk.close()
        return
    kernel_lines(hk, a.n, max(a.reps, 3), [int(s) for s in a.sizes.split(",")])
    hk.close()


if __name__ == "__main__":
    main()
