"""Timings of kernel ridge regression on points of more than 64 coordinates (profiles/kernel_highdim.md), one measurement per
process so that each runs under its own time limit:

  python tools/kernel_highdim_bench.py knn     --n 100000 --d 128 [--k 64] [--reps 3]
  python tools/kernel_highdim_bench.py predict --n 100000 --m 10000 --d 128 [--type 0] [--reps 3]
  python tools/kernel_highdim_bench.py fit     --n 100000 --d 128 [--rel_tol 1e-2] [--leaf 128]

knn:     hssk_knn over all points (cluster order) on the device clock (stopwatch slot 7, the one the compression brackets the search
         with); ms, ms per coordinate, and for the filtered form the fraction of the FP32 matrix-core roof its 2 n^2 (d + 2) flops
         reach.  HSSK_KNN_FILTER=0 in the environment gives the heap / general form.
predict: hssk_kernel_predict (FP64) and hssk_kernel_predict_f32 / _wide (FP32) on the same points; ms and pairs x coordinates / s.
fit:     STRUMPACK_kernel_fit_HSS_double end to end (wall clock) with the stage split of SPX_kernel_fit_info.
The points: a few Gaussian clusters with a low-dimensional spread, embedded by a random rotation (the data of the tests).
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

PEAK_FP32_MFMA_TFLOPS = 157.3


def clustered_points(seed, n, d, clusters=8, latent=4):
    r = np.random.default_rng(seed)
    Q = np.linalg.qr(r.standard_normal((d, d)))[0][:, :latent]
    centres = r.standard_normal((clusters, d))
    lab = r.integers(0, clusters, n)
    X = centres[lab] + (r.standard_normal((n, latent)) * np.sqrt(d / latent)) @ Q.T + 0.01 * r.standard_normal((n, d))
    return X, np.where(lab % 2 == 0, 1.0, -1.0)


def watches(lib):
    lib.hssk_watch_start.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_stop.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_read_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.hssk_watch_read_ms.restype = C.c_double


def run_knn(a):
    lib = KM.load(_loader.lib_path())
    X, _ = clustered_points(2025, a.n, a.d)
    Xp, perm, leaves = KM.clustering(lib, X, "cobble", 256)
    hk = K.Hssk(_loader.lib_path())
    watches(hk.lib)
    dX = hk.array(Xp.T)
    out = hk.empty((a.k, a.n), dtype=np.int32)
    ms = []
    c0 = hk.lib.hssk_knn_filtered_count(hk.ctx) if hasattr(hk.lib, "hssk_knn_filtered_count") else 0
    for rep in range(a.reps + 1):
        hk.check(hk.lib.hssk_watch_start(hk.ctx, 7))
        hk.check(hk.lib.hssk_knn(hk.ctx, dX.ptr, a.d, a.n, a.k, 0, a.n, out.ptr))
        hk.check(hk.lib.hssk_watch_stop(hk.ctx, 7))
        hk.sync()
        v = hk.lib.hssk_watch_read_ms(hk.ctx, 7, None)
        if rep:
            ms.append(v)
    filtered = (hk.lib.hssk_knn_filtered_count(hk.ctx) - c0) > 0 if hasattr(hk.lib, "hssk_knn_filtered_count") else None
    best = min(ms)
    tf = 2.0 * a.n * a.n * (a.d + 2) / (best * 1e-3) * 1e-12
    print(json.dumps(dict(what="knn", n=a.n, d=a.d, k=a.k, filtered=filtered, ms_min=round(best, 3), ms_max=round(max(ms), 3),
                          ms_per_coordinate=round(best / a.d, 4), tflops=round(tf, 2),
                          fp32_mfma_roof_fraction=round(tf / PEAK_FP32_MFMA_TFLOPS, 4) if filtered else None,
                          neighbours_checksum=int(np.sort(out.get().T[:64], axis=1).sum()))), flush=True)
    hk.close()


def run_predict(a):
    hk = K.Hssk(_loader.lib_path())
    lib = hk.lib
    watches(lib)
    r = np.random.default_rng(7)
    X, T, w = r.standard_normal((a.n, a.d)).astype(np.float32), r.standard_normal((a.m, a.d)).astype(np.float32), r.standard_normal(a.n).astype(np.float32)
    h = {0: 0.9 * np.sqrt(a.d) + 0.4, 1: 0.9 * a.d, 2: 0.9 * np.sqrt(a.d) + 0.4}[a.type]
    p = min(8, a.d) if a.type == 2 else 1
    work = float(a.n) * a.m * a.d
    fX, fT, fw, fp = hk.array(X.ravel()), hk.array(T.ravel()), hk.array(w), hk.empty((a.m,), np.float32)
    fn = lib.hssk_kernel_predict_f32 if a.d <= 64 else lib.hssk_kernel_predict_f32_wide
    st = np.zeros(6, dtype=np.int64)
    us = []
    for it in range(a.reps + 1):
        hk.check(fn(hk.ctx, fX.ptr, a.n, a.d, a.type, p, float(h), fw.ptr, fT.ptr, a.m, fp.ptr, st.ctypes.data))
        if it:
            us.append((int(st[3]), int(st[0]), int(st[1])))
    pf = fp.get().astype(np.float64)
    best = min(us)
    print(json.dumps(dict(what="predict", kind="fp32", type=a.type, n=a.n, m=a.m, d=a.d, ms_min=round(best[0] * 1e-3, 3),
                          mfma_tiles=best[1], diff_tiles=best[2], pair_coordinates_per_s=round(work / (best[0] * 1e-6), 0))), flush=True)
    for arr in (fX, fT, fw, fp):
        arr.free()
    dX, dT, dw, dp = hk.array(X.astype(np.float64).ravel()), hk.array(T.astype(np.float64).ravel()), hk.array(w.astype(np.float64)), hk.empty((a.m,))
    spec = K.KernelSpec(dX.ptr, a.n, a.d, a.type, p, float(h), 0.0)
    ms = []
    for it in range(a.reps + 1):
        hk.check(lib.hssk_watch_start(hk.ctx, 0))
        hk.check(lib.hssk_kernel_predict(hk.ctx, C.byref(spec), dw.ptr, dT.ptr, a.m, dp.ptr))
        hk.check(lib.hssk_watch_stop(hk.ctx, 0))
        hk.sync()
        v = lib.hssk_watch_read_ms(hk.ctx, 0, None)
        if it:
            ms.append(v)
    pd = dp.get()
    print(json.dumps(dict(what="predict", kind="fp64", type=a.type, n=a.n, m=a.m, d=a.d, ms_min=round(min(ms), 3),
                          pair_coordinates_per_s=round(work / (min(ms) * 1e-3), 0),
                          fp32_vs_fp64_rel_diff=float(np.linalg.norm(pf - pd) / np.linalg.norm(pd)))), flush=True)
    hk.close()


def run_fit(a):
    lib = KM.load(_loader.lib_path())
    X, y = clustered_points(2025, a.n, a.d)
    kr = KM.KernelRegression(lib, h=float(np.sqrt(a.d)), lam=1.0, kernel="Gauss",
                             argv=["--hss_leaf_size", str(a.leaf), "--hss_rel_tol", str(a.rel_tol)])
    t0 = time.perf_counter()
    kr.fit(X, y)
    wall = (time.perf_counter() - t0) * 1e3
    info = kr.info()
    print(json.dumps(dict(what="fit", n=a.n, d=a.d, rel_tol=a.rel_tol, leaf=a.leaf, wall_ms=round(wall, 1), compressed=info["compressed"],
                          rank=info["rank"], levels=info["levels"], memory_MB=round(info["memory"] / 1e6, 1),
                          compress_ms=round(info["compress_us"] * 1e-3, 1), factor_ms=round(info["factor_us"] * 1e-3, 1),
                          solve_ms=round(info["solve_us"] * 1e-3, 1))), flush=True)
    kr.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["knn", "predict", "fit"])
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--type", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rel_tol", type=float, default=1e-2)
    ap.add_argument("--leaf", type=int, default=128)
    a = ap.parse_args()
    {"knn": run_knn, "predict": run_predict, "fit": run_fit}[a.what](a)


if __name__ == "__main__":
    main()
