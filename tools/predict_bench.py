"""Timing of the single-precision prediction kernel against the FP64 one, in one process on one GPU:

  * hssk_kernel_predict_f32 (device-clock brackets of its own launches: all, main, prep + reduce) and hssk_kernel_predict on the
    widened copy of the same points (a device-clock stopwatch, hssk_watch_*), minimum over --reps calls after two warm-up calls;
  * with --api: a float fit of the susy set through STRUMPACK_*_float, then the wall-clock time of the first and of the second
    STRUMPACK_kernel_predict_float with the statistics of SPX_kernel_predict_stats.

  python tools/predict_bench.py --shape uniform8_m64|uniform8_m1000|uniform8_m100000|susy10k|laplace|anova [--reps 5] [--api]

One shape per process (run each under its own time limit).  HSSK_KPREDICT_FORCE_DIFF=1 in the environment gives the A/B line of
the Gauss route: everything in the difference form.  Prints one JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from strumpack_amd import _loader  # noqa: E402
from strumpack_amd import hssk as K  # noqa: E402
from strumpack_amd import kernel as KM  # noqa: E402

CLOCK_GHZ, SIMDS = 2.4, 1024      # nominal shader clock and SIMDs of an MI355X: the yardstick of the exponential-issue floor
SHAPES = {   # name: (kernel type, degree, h, n, m, data)
    "uniform8_m64": (0, 1, 1.3, 100000, 64, "uniform"),
    "uniform8_m1000": (0, 1, 1.3, 100000, 1000, "uniform"),
    "uniform8_m100000": (0, 1, 1.3, 100000, 100000, "uniform"),
    "susy10k": (0, 1, 1.3, 10000, 1000, "susy"),
    "laplace": (1, 1, 1.3, 100000, 1000, "uniform"),
    "anova": (2, 2, 1.3, 100000, 1000, "uniform"),
}


def points(data, n, m):
    if data == "susy":
        import kernel_golden as KG
        X, y, T, yt = KG.susy()
        Z = np.load(os.path.join(KG.GOLD, "kernel_golden.npz"))
        return X[:n][Z["perm_gauss_10k"] - 1].astype(np.float32), T[:m].astype(np.float32), Z["weights_gauss_10k"].astype(np.float32)
    r = np.random.default_rng(2025)
    return r.random((n, 8), dtype=np.float32), r.random((m, 8), dtype=np.float32), r.standard_normal(n).astype(np.float32)


def kernel_lines(hk, name, reps):
    kt, p, h, n, m, data = SHAPES[name]
    lib = hk.lib
    lib.hssk_watch_start.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_stop.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_read_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.hssk_watch_read_ms.restype = C.c_double
    X, T, w = points(data, n, m)
    d = X.shape[1]
    pairs = float(n) * m
    exps = pairs * (d if kt == 2 else 1)
    floor_ms = exps / 64 * 16 / SIMDS / (CLOCK_GHZ * 1e9) * 1e3   # one quarter-rate v_exp_f32 per wave and 64 exponentials
    fX, fT, fw, fp = hk.array(X.ravel()), hk.array(T.ravel()), hk.array(w), hk.empty((m,), np.float32)
    st = np.zeros(6, dtype=np.int64)
    runs = []
    for it in range(reps + 2):
        hk.check(lib.hssk_kernel_predict_f32(hk.ctx, fX.ptr, n, d, kt, p, h, fw.ptr, fT.ptr, m, fp.ptr, st.ctypes.data))
        if it >= 2:
            runs.append(st.copy())
    pf = fp.get().astype(np.float64)
    all_us = [int(s[3]) for s in runs]
    best = runs[int(np.argmin(all_us))]
    f32_ms = min(all_us) * 1e-3
    print(json.dumps(dict(what="predict_kernel", kind="fp32", shape=name, type=kt, n=n, m=m, d=d, reps=reps,
                          forced_diff=os.environ.get("HSSK_KPREDICT_FORCE_DIFF") == "1",
                          ms_min=round(f32_ms, 4), ms_max=round(max(all_us) * 1e-3, 4), main_ms=round(int(best[4]) * 1e-3, 4),
                          prep_reduce_ms=round(int(best[5]) * 1e-3, 4), mfma_tiles=int(best[0]), diff_tiles=int(best[1]),
                          splits=int(best[2]), gpairs_per_s=round(pairs / (f32_ms * 1e-3) * 1e-9, 2),
                          exp_floor_ms=round(floor_ms, 4), exp_floor_fraction=round(floor_ms / (int(best[4]) * 1e-3), 3))), flush=True)
    for a in (fX, fT, fw):
        a.free()
    dX, dT, dw, dp = hk.array(X.astype(np.float64).ravel()), hk.array(T.astype(np.float64).ravel()), hk.array(w.astype(np.float64)), hk.empty((m,))
    spec = K.KernelSpec(dX.ptr, n, d, kt, p, h, 0.0)
    ms = []
    for it in range(reps + 2):
        hk.check(lib.hssk_watch_start(hk.ctx, 0))
        hk.check(lib.hssk_kernel_predict(hk.ctx, C.byref(spec), dw.ptr, dT.ptr, m, dp.ptr))
        hk.check(lib.hssk_watch_stop(hk.ctx, 0))
        v = lib.hssk_watch_read_ms(hk.ctx, 0, None)
        if it >= 2:
            ms.append(v)
    pd = dp.get()
    print(json.dumps(dict(what="predict_kernel", kind="fp64", shape=name, type=kt, n=n, m=m, d=d, reps=reps, ms_min=round(min(ms), 4),
                          ms_max=round(max(ms), 4), gpairs_per_s=round(pairs / (min(ms) * 1e-3) * 1e-9, 2))), flush=True)
    print(json.dumps(dict(what="predict_ratio", shape=name, fp64_over_fp32=round(min(ms) / f32_ms, 2),
                          worst_case_ratio=round(min(ms) / (max(all_us) * 1e-3), 2),
                          rel_diff=float(np.linalg.norm(pf - pd) / np.linalg.norm(pd)))), flush=True)


def api_lines(reps):
    import kernel_golden as KG
    J, Z = KG.golden()
    g = J["regression_gauss_10k"]
    X, y, T, yt = KG.susy()
    lib = KM.load(_loader.lib_path())
    kr = KM.KernelRegression(lib, h=g["h"], lam=g["lam"], kernel="rbf", argv=KG.fit_args(g))
    t0 = time.perf_counter()
    kr.fit(X[:g["n"]].astype(np.float32), y[:g["n"]].astype(np.float32))
    fit_ms = (time.perf_counter() - t0) * 1e3
    Tf = T[:g["m"]].astype(np.float32)
    calls = []
    for it in range(reps + 1):
        t0 = time.perf_counter()
        pred = kr.decision_function(Tf)
        calls.append(((time.perf_counter() - t0) * 1e3, kr.predict_stats()))
    acc = float(np.mean((pred >= 0) == (yt[:g["m"]] >= 0)))
    print(json.dumps(dict(what="predict_float_api", n=g["n"], m=g["m"], fit_ms=round(fit_ms, 1), first_call_ms=round(calls[0][0], 3),
                          second_call_ms=round(calls[1][0], 3), later_min_ms=round(min(c[0] for c in calls[1:]), 3),
                          first_stats=calls[0][1], second_stats=calls[1][1], accuracy=acc)), flush=True)
    kr.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="susy10k", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--api", action="store_true")
    a = ap.parse_args()
    if a.api:
        api_lines(max(a.reps, 2))
        return
    hk = K.Hssk(_loader.lib_path())
    kernel_lines(hk, a.shape, max(a.reps, 3))
    hk.close()


if __name__ == "__main__":
    main()
