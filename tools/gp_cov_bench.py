"""Timing of the joint predictive covariance and of its two kernels, in one process on one GPU (profiles/gp_covariance.md):

  * --sweep: hssk_kernel_cross_matmul (nc = 64) and hssk_kernel_cross_split at N training points uniform in [0, 1)^8, Gauss and
    Laplace, h = 1.3, m = 64, 1024 and 4096 test points, with forced split counts around the automatic ones (what the constants
    behind hssk_kernel_cross_matmul_splits and hssk_kernel_cross_splits were chosen from).  At m = 4096 also hssk_kernel_matmul
    with 64 columns: the square product of the same stage loop, as pairs per second and as a fraction of the FP64 matrix roof
    (hssk_mfma_f64_peak_tflops of the same run; 128 flops per pair at 64 columns).  At m = 64 also hssk_kernel_cross and
    hssk_kernel_predict_cols, the two kernels of a variance chunk.
  * --model: a kept Gauss fit of the same points (rel_tol 1e-2), then predict_variance and predict_covariance of the same 64 test
    points with the device-clock parts of SPX_kernel_variance_ms and SPX_kernel_covariance_ms, and predict_covariance of 1024 and
    4096 test points with its three parts and the host clock.

Device-clock stopwatches (hssk_watch_*) around each call, two warm-up calls, then --reps calls: minimum, median, maximum.

  python tools/gp_cov_bench.py [--n 100000] [--reps 5] (--sweep | --model)

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

H, D, NC = 1.3, 8, 64
KINDS = (("gauss", 0), ("laplace", 1))
WATCH = 0


def stats(ms):
    return dict(ms_min=round(min(ms), 4), ms_median=round(float(np.median(ms)), 4), ms_max=round(max(ms), 4))


def timed(hk, f, reps):
    lib, ms = hk.lib, []
    for it in range(reps + 2):
        hk.check(lib.hssk_watch_start(hk.ctx, WATCH))
        hk.check(f())
        hk.check(lib.hssk_watch_stop(hk.ctx, WATCH))
        v = lib.hssk_watch_read_ms(hk.ctx, WATCH, None)
        if it >= 2:
            ms.append(v)
    return ms


def sweep_lines(hk, n, reps, sizes):
    lib = hk.lib
    lib.hssk_watch_start.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_stop.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_read_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.hssk_watch_read_ms.restype = C.c_double
    lib.hssk_mfma_f64_peak_tflops.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_mfma_f64_peak_tflops.restype = C.c_double
    peak = float(lib.hssk_mfma_f64_peak_tflops(hk.ctx, 20000))
    print(json.dumps(dict(what="mfma_f64_peak_tflops", value=round(peak, 2))), flush=True)
    r = np.random.default_rng(2025)
    dX, dB = hk.array(r.random((n, D)).ravel()), hk.array(r.standard_normal((n, NC)))
    stages, tiles_n = (n + 15) // 16, (n + 63) // 64
    for m in sizes:
        dT, dO, dK = hk.array(r.random((m, D)).ravel()), hk.empty((m, NC)), hk.empty((n, min(m, 64)))
        tiles = (m + 63) // 64
        for name, kt in KINDS:
            spec = K.KernelSpec(dX.ptr, n, D, kt, 1, H, 0.0)
            out = {}
            for wgs in (128, 256, 512, 768, 1024, 1536, 2048, 4096, 8192):
                s = max(1, min(stages, -(-wgs // tiles)))
                if s in out:
                    continue
                ms = timed(hk, lambda: lib.hssk_kernel_cross_matmul(hk.ctx, C.byref(spec), dT.ptr, m, dB.ptr, n, NC, dO.ptr, m, s), reps)
                out[s] = dict(workgroups=s * tiles, gpairs_per_s=round(float(n) * m / (min(ms) * 1e-3) * 1e-9, 2), **stats(ms))
            ms = timed(hk, lambda: lib.hssk_kernel_cross_matmul(hk.ctx, C.byref(spec), dT.ptr, m, dB.ptr, n, NC, dO.ptr, m, 0), reps)
            rate = float(n) * m / (min(ms) * 1e-3)
            print(json.dumps(dict(what="cross_matmul_split_sweep", kernel=name, n=n, m=m, nc=NC, d=D, reps=reps,
                                  automatic=int(lib.hssk_kernel_cross_matmul_splits(n, m)), automatic_ms=stats(ms),
                                  automatic_gpairs_per_s=round(rate * 1e-9, 2), automatic_roof_fraction=round(rate * 2 * NC * 1e-12 / peak, 4),
                                  splits=out)), flush=True)
            # the cross block of a chunk of (at most) 64 of these test points
            mc = min(m, 64)
            out = {}
            for wgs in (64, 256, 512, 1024, 2048, 4096):
                s = max(1, min(tiles_n, wgs))
                if s in out:
                    continue
                ms = timed(hk, lambda: lib.hssk_kernel_cross_split(hk.ctx, C.byref(spec), dT.ptr, mc, dK.ptr, n, s), reps)
                out[s] = dict(workgroups=s, **stats(ms))
            ms = timed(hk, lambda: lib.hssk_kernel_cross_split(hk.ctx, C.byref(spec), dT.ptr, mc, dK.ptr, n, 0), reps)
            line = dict(what="cross_split_sweep", kernel=name, n=n, m=mc, d=D, reps=reps, automatic=int(lib.hssk_kernel_cross_splits(n, mc)),
                        automatic_ms=stats(ms), splits=out)
            if m == 64:
                dP = hk.empty((64,))
                line["kernel_cross"] = stats(timed(hk, lambda: lib.hssk_kernel_cross(hk.ctx, C.byref(spec), dT.ptr, mc, dK.ptr, n), reps))
                line["kernel_predict_cols"] = stats(timed(hk, lambda: lib.hssk_kernel_predict_cols(hk.ctx, C.byref(spec), dB.ptr, n, dT.ptr, mc, dP.ptr), reps))
                dP.free()
            print(json.dumps(line), flush=True)
            if m >= 4096:
                dS = hk.empty((n, NC))
                ms = timed(hk, lambda: lib.hssk_kernel_matmul(hk.ctx, C.byref(spec), 0, dB.ptr, n, NC, dS.ptr, n, 0), max(3, reps // 2))
                rate = float(n) * n / (min(ms) * 1e-3)
                print(json.dumps(dict(what="kernel_matmul_square", kernel=name, n=n, nc=NC, d=D, **stats(ms), gpairs_per_s=round(rate * 1e-9, 2),
                                      roof_fraction=round(rate * 2 * NC * 1e-12 / peak, 4))), flush=True)
                dS.free()
        for a in (dT, dO, dK):
            a.free()
    dX.free()
    dB.free()


def model_lines(n, reps, sizes):
    lib = KM.load(_loader.lib_path())
    r = np.random.default_rng(2025)
    X = r.random((n, D))
    y = np.sign((X - 0.5) @ r.standard_normal(D))
    argv = ["--hss_leaf_size", "128", "--hss_rel_tol", "1e-2", "--hss_abs_tol", "1e-8", "--hss_approximate_neighbors", "64"]
    kr = KM.KernelRegression(lib, h=H, lam=3.11, kernel="rbf", argv=argv, keep_model=True).fit(X, y)
    T = r.random((64, D))
    var, cov, wall = [], [], {"variance": [], "covariance": []}
    for it in range(reps + 2):
        t0 = time.perf_counter()
        v = kr.predict_variance(T)
        t1 = time.perf_counter()
        pv = kr.variance_ms()
        t2 = time.perf_counter()
        c = kr.predict_covariance(T)
        t3 = time.perf_counter()
        pc = kr.covariance_ms()
        assert np.array_equal(c, c.T) and np.abs(np.diag(c) - v).max() < 1e-9
        if it >= 2:
            var.append(pv)
            cov.append(pc)
            wall["variance"].append((t1 - t0) * 1e3)
            wall["covariance"].append((t3 - t2) * 1e3)
    vt, ct = [sum(p.values()) for p in var], [sum(p.values()) for p in cov]
    print(json.dumps(dict(what="covariance_chunk_against_variance", n=n, m=64, d=D, reps=reps,
                          variance_device_ms=stats(vt), covariance_device_ms=stats(ct),
                          variance_parts_ms=var[int(np.argmin(vt))], covariance_parts_ms=cov[int(np.argmin(ct))],
                          variance_host_ms=stats(wall["variance"]), covariance_host_ms=stats(wall["covariance"]),
                          covariance_over_variance=round(min(ct) / min(vt), 5))), flush=True)
    for m in sizes:
        T = r.random((m, D))
        parts, host = [], []
        for it in range(3):
            t0 = time.perf_counter()
            c = kr.predict_covariance(T)
            host.append((time.perf_counter() - t0) * 1e3)
            parts.append(kr.covariance_ms())
        assert np.array_equal(c, c.T)
        tot = [sum(p.values()) for p in parts[1:]]
        print(json.dumps(dict(what="joint_covariance", n=n, m=m, d=D, device_ms=stats(tot), parts_ms=parts[1 + int(np.argmin(tot))],
                              host_ms=stats(host[1:]), smallest_eigenvalue=float(np.linalg.eigvalsh(c).min()) if m <= 1024 else None)), flush=True)
    kr.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    if a.model:
        model_lines(a.n, max(a.reps, 3), [int(s) for s in (a.sizes or "1024,4096").split(",")])
        return
    hk = K.Hssk(_loader.lib_path())
    sweep_lines(hk, a.n, max(a.reps, 3), [int(s) for s in (a.sizes or "64,1024,4096").split(",")])
    hk.close()


if __name__ == "__main__":
    main()
