"""Timing of the single-precision sketch against the FP64 sketch, in one process on one GPU:

  * hssk_dgemm on the FP64 Toeplitz operand and hssk_sgemm_sketch on its narrowed copy, m = 192, both transB, per size
    (the whole call on a device-clock stopwatch, hssk_watch_*, and the bracket of its main launch, hssk_last_dgemm_ms);
  * a whole SPX_s_struct_from_dense_device (precision 1) step against SPX_d_struct_from_dense_device on the widened operand.

  python tools/f32_sketch_bench.py [--sizes 32768,100000] [--reps 5] [--step-n 32768]

Prints one JSON line per measurement; the yardstick is the FP64 line of the same run."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from strumpack_amd import _loader, capi  # noqa: E402
from strumpack_amd import hssk as K  # noqa: E402

FP64_PEAK, FP32_PEAK = 78.6, 157.3   # TFLOP/s, matrix cores of gfx950


def gemm_lines(hk, n, reps, m=192):
    lib = hk.lib
    lib.hssk_watch_start.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_stop.argtypes = [C.c_void_p, C.c_int]
    lib.hssk_watch_read_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.hssk_watch_read_ms.restype = C.c_double
    d64 = hk.empty((n, n))
    hk.check(lib.hssk_fill_toeplitz(hk.ctx, d64.ptr, n, n, b"T"))
    d32 = hk.empty((n, n), dtype=np.float32)
    hk.check(lib.hssk_narrow_f32(hk.ctx, d32.ptr, n, d64.ptr, n, n, n))
    dR = hk.empty((m, n))
    hk.check(lib.hssk_randn(hk.ctx, dR.ptr, m, n, m, 0, n, 1234))
    dC = hk.empty((m, n))
    hk.sync()
    for tb in (1, 0):
        for kind in ("fp64", "fp32"):
            def call():
                if kind == "fp64":
                    hk.check(lib.hssk_dgemm(hk.ctx, tb, m, n, n, 1.0, dR.ptr, m, d64.ptr, n, 0.0, dC.ptr, m))
                else:
                    hk.check(lib.hssk_sgemm_sketch(hk.ctx, tb, m, n, n, 1.0, dR.ptr, m, d32.ptr, n, 0.0, dC.ptr, m))
            for _ in range(2):
                call()
            hk.sync()
            main_ms, main_fl = [], 0.0
            for _ in range(reps):
                hk.check(lib.hssk_watch_start(hk.ctx, 0))
                call()
                hk.check(lib.hssk_watch_stop(hk.ctx, 0))
                hk.sync()
                main_ms.append(float(lib.hssk_last_dgemm_ms(hk.ctx)))
                main_fl = float(lib.hssk_last_dgemm_flops(hk.ctx))
            pairs = C.c_int()
            call_ms = lib.hssk_watch_read_ms(hk.ctx, 0, C.byref(pairs)) / max(pairs.value, 1)
            mm = float(np.mean(main_ms))
            peak = FP64_PEAK if kind == "fp64" else FP32_PEAK
            line = dict(what="sketch_product", kind=kind, n=n, m=m, transB=tb, reps=reps, call_ms=round(call_ms, 4),
                        call_tflops=round(2.0 * m * n * n / (call_ms * 1e-3) * 1e-12, 2),
                        main_ms=round(mm, 4), main_ms_min=round(min(main_ms), 4), main_ms_max=round(max(main_ms), 4),
                        main_tflops=round(main_fl / (mm * 1e-3) * 1e-12, 2),
                        main_roof_fraction=round(main_fl / (mm * 1e-3) * 1e-12 / peak, 3))
            print(json.dumps(line), flush=True)
    for d in (d64, d32, dR, dC):
        d.free()


def step_lines(L, hk, n, reps):
    lib = hk.lib
    d64 = hk.empty((n, n))
    hk.check(lib.hssk_fill_toeplitz(hk.ctx, d64.ptr, n, n, b"T"))
    d32 = hk.empty((n, n), dtype=np.float32)
    hk.check(lib.hssk_narrow_f32(hk.ctx, d32.ptr, n, d64.ptr, n, n, n))
    hk.check(lib.hssk_expand_image(hk.ctx, d64.ptr, n, d32.ptr, n, n, n, 1))   # the widened float operand
    hk.sync()
    for rtol in (1e-2, 1e-4):
        o = capi.CSPOptions()
        L.SP_s_struct_default_options(C.byref(o))
        o.type, o.rel_tol, o.abs_tol, o.leaf_size, o.max_rank, o.verbose = 0, rtol, 1e-8, 256, 50000, 0
        for kind in ("fp64", "fp32"):
            ts, st, rank = [], None, 0
            for it in range(reps + 1):   # (the first one warms up)
                t0 = time.perf_counter()
                if kind == "fp64":
                    H = capi.StructuredMatrix.from_dense_device(L, d64.ptr, n, n, o, None)
                else:
                    H = capi.StructuredMatrixF32.from_dense_device(L, d32.ptr, n, n, o, None, 1)
                dt = time.perf_counter() - t0
                if it:
                    ts.append(dt * 1e3)
                st, rank = H.stats(), H.rank()
                H.destroy()
            line = dict(what="compress_step", kind=kind, n=n, leaf=256, rel_tol=rtol, reps=reps, step_ms=round(float(np.mean(ts)), 3),
                        step_ms_min=round(min(ts), 3), step_ms_max=round(max(ts), 3), rank=rank,
                        sketch_kernel_ms=round(st["sketch_kernel_ms"], 3), sketch_launches=int(st["sketch_launches"]),
                        t_sketch_ms=round(st["t_sketch"] * 1e3, 3), rounds=int(st["rounds"]))
            print(json.dumps(line), flush=True)
    d64.free()
    d32.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32768")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-n", type=int, default=32768)
    a = ap.parse_args()
    hk = K.Hssk(_loader.lib_path())
    L = capi.load(_loader.lib_path())
    for n in [int(s) for s in a.sizes.split(",") if s]:
        gemm_lines(hk, n, max(a.reps, 5))
    if a.step_n > 0:
        step_lines(L, hk, a.step_n, max(a.reps, 5))
    hk.close()


if __name__ == "__main__":
    main()
