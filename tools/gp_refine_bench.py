"""What the solves with the exact kernel matrix cost next to the fit they start from (profiles/gp_refine.md).

One process, the workload of tools/gp_grad_bench.py: N points uniform in [0, 1)^8, Gauss kernel h = 1.3, lambda = 3.11, cobble
clustering, leaf 128, 64 neighbours.  Needs the GPU (the product library; no fallback).

  refine         KernelRegression.refine at the compression tolerances 1e-2 and 1e-4 and rtol 1e-6 and 1e-8, defaults otherwise
                 (maxit 100, restart 30), each from the compressed weights (set_lambda with the same lambda restores them): the
                 residual before and after, steps, products, host clock and the device-event split (SPX_kernel_krylov_ms)
  variance       one chunk of 64 test points through predict_variance(exact=True) next to the compressed predict_variance
  kernels        hssk_krylov_orth alone at nc = 1 and 64, k = 0 and 29, against hssk_kernel_matmul with the same nc in the same run
                 (device events), and the bytes a CGS2 step asks for.  Per row and column, 8 bytes times: the k + 1 blocks four
                 times (the dots once, the first update twice -- once to update, once for the dots of the new w --, the second
                 update once) and w seven times (read by each of the four launches, written by both updates, and block k + 1
                 written by the finish): 4 (k + 1) + 7

    python tools/gp_refine_bench.py --n 100000 --out gp_refine_bench.json --md gp_refine.md
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COMPRESSED_SOLVE_MS, PAIR_KERNEL_MS = 0.77, (54.0, 62.0)   # 64 columns; cross / column-sum kernels of a chunk (profiles/gp_variance.md)
PARENT_FIT_MS = 22.2                                       # profiles/gp_variance.md


def refine_runs(KM, lib, X, y, h, lam, leaf, rel_tol, rtols):
    argv = ["--hss_leaf_size", str(leaf), "--hss_rel_tol", "%g" % rel_tol, "--hss_abs_tol", "1e-8", "--hss_approximate_neighbors", "64"]
    kr = KM.KernelRegression(lib, h=h, lam=lam, kernel="rbf", argv=argv, keep_model=True)
    fits = []
    for _ in range(3):                              # (the first fit of a process loads code objects and fills the device pool)
        t0 = time.perf_counter()
        kr.fit(X, y)
        fits.append((time.perf_counter() - t0) * 1e3)
    out = {"rel_tol": rel_tol, "fit_ms": fits, "rank": kr.info()["rank"], "fit_residual": kr.fit_residual(), "runs": []}
    for rtol in rtols:
        kr.set_lambda(lam)                          # the compressed weights again
        t0 = time.perf_counter()
        info = kr.refine(rtol=rtol)
        wall = (time.perf_counter() - t0) * 1e3
        out["runs"].append(dict(rtol=rtol, host_ms=wall, ms=kr.krylov_ms(), converged=info["converged"], iterations=info["iterations"],
                                products=info["products"], solves=info["solves"], cycles=info["cycles"], residual0=info["residual0"],
                                residual=info["residual"]))
    # one chunk of 64 test points
    T = np.random.default_rng(7).random((64, X.shape[1]))
    kr.set_lambda(lam)
    t0 = time.perf_counter()
    vc = kr.predict_variance(T)
    out["variance_compressed"] = dict(host_ms=(time.perf_counter() - t0) * 1e3, ms=kr.variance_ms(), min=float(vc.min()), max=float(vc.max()))
    out["variance_exact"] = []
    for rtol in rtols:
        t0 = time.perf_counter()
        ve, info = kr.predict_variance(T, exact=True, rtol=rtol, info=True)
        out["variance_exact"].append(dict(rtol=rtol, host_ms=(time.perf_counter() - t0) * 1e3, ms=kr.krylov_ms(), converged=info["converged"],
                                          iterations=info["iterations"], products=info["products"], solves=info["solves"],
                                          residual0=info["residual0"], residual_max=info["residual_max"], min=float(ve.min()),
                                          max=float(ve.max()), gap=float(np.abs(ve - vc).max())))
    kr.destroy()
    return out


def kernel_runs(n, reps=5):
    """hssk_krylov_orth and hssk_kernel_matmul on their own: device events"""
    from strumpack_amd import _loader
    from strumpack_amd import hssk as K
    hk = K.Hssk(_loader.lib_path())
    L = hk.lib
    L.hssk_watch_start.argtypes = L.hssk_watch_stop.argtypes = [C.c_void_p, C.c_int]
    L.hssk_watch_read_ms.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.hssk_watch_read_ms.restype = C.c_double
    d, res = 8, []
    dX = hk.array(np.random.default_rng(1).random((d, n)))
    spec = K.KernelSpec(dX.ptr, n, d, 0, 1, 1.3, 3.11)
    for nc in (1, 64):
        dV, dW, dO, dH = hk.empty((n, nc, 31)), hk.empty((n, nc)), hk.empty((n, nc)), hk.empty((32, nc))
        hk.check(L.hssk_randn(hk.ctx, dV.ptr, n, nc * 31, n, 0, nc * 31, 5))
        active = (1 << nc) - 1
        for k in (0, 29):
            for timed in (False, True):             # (one untimed call first)
                for _ in range(reps if timed else 1):
                    hk.check(L.hssk_randn(hk.ctx, dW.ptr, n, nc, n, 0, nc, 9))
                    L.hssk_watch_start(hk.ctx, 1)
                    hk.check(L.hssk_krylov_orth(hk.ctx, dV.ptr, n, n, nc, k, dW.ptr, n, active, dH.ptr, 32))
                    L.hssk_watch_stop(hk.ctx, 1)
                    L.hssk_watch_start(hk.ctx, 2)
                    hk.check(L.hssk_kernel_matmul(hk.ctx, C.byref(spec), 0, dW.ptr, n, nc, dO.ptr, n, 0))
                    L.hssk_watch_stop(hk.ctx, 2)
                orth, prod = L.hssk_watch_read_ms(hk.ctx, 1, None) / reps, L.hssk_watch_read_ms(hk.ctx, 2, None) / reps
            gbytes = 8.0 * n * nc * (4 * (k + 1) + 7) / 1e9      # (the count of the module's docstring)
            res.append(dict(nc=nc, k=k, orth_ms=orth, product_ms=prod, gbytes=gbytes, tb_per_s=gbytes / orth, share=orth / (orth + prod)))
        for v in (dV, dW, dO, dH):
            v.free()
    dX.free()
    hk.close()
    return res


def markdown(r):
    n = r["n"]
    lines = [
        "# Exact-kernel weights and variances: GMRES on the kept HSS fit",
        "",
        "Tool: `tools/gp_refine_bench.py` (one process; the workload of `tools/gp_grad_bench.py`: N = %d points uniform in [0, 1)^8, Gauss," % n,
        "h = 1.3, lambda = 3.11, cobble, leaf %d, 64 neighbours).  Host clocks around calls that end in a device synchronise; the split" % r["leaf"],
        "of a call comes from device events around its products, ULV solves and Krylov kernels.  Defaults: maxit 100, restart 30.",
        "",
        "## refine",
        "",
        "| rel_tol | fit (third, host) | rank | rtol | residual before | steps | products | cycles | residual after | converged | host | products | solves | Krylov kernels |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for f in r["fits"]:
        for q in f["runs"]:
            lines.append("| %g | %.1f ms | %d | %g | %.3g | %d | %d | %d | %.3g | %s | %.0f ms | %.0f ms | %.1f ms | %.1f ms |"
                         % (f["rel_tol"], f["fit_ms"][-1], f["rank"], q["rtol"], q["residual0"], q["iterations"], q["products"], q["cycles"],
                            q["residual"], "yes" if q["converged"] else "no", q["host_ms"], q["ms"]["product_ms"], q["ms"]["solve_ms"],
                            q["ms"]["krylov_ms"]))
    lines += ["", "(The parent commit's fit: %.1f ms.  `fit_residual` of the two fits: %s.)"
              % (PARENT_FIT_MS, ", ".join("%.3g at rel_tol %g" % (f["fit_residual"], f["rel_tol"]) for f in r["fits"])), ""]
    for f in r["fits"]:
        for q in f["runs"]:
            lines.append("- rel_tol %g, rtol %g: fit %.0f ms + refine %.0f ms = %.0f ms; %s."
                         % (f["rel_tol"], q["rtol"], f["fit_ms"][-1], q["host_ms"], f["fit_ms"][-1] + q["host_ms"],
                            "converged in %d steps" % q["iterations"] if q["converged"] else
                            "NOT converged: the %d steps of maxit took the residual from %.3g to %.3g" % (q["iterations"], q["residual0"], q["residual"])))
    lines += ["",
              "## One variance chunk of 64 test points", "",
              "Next to it: the compressed solve of a chunk is %.2f ms and its two pair kernels %.0f and %.0f ms (`profiles/gp_variance.md`)."
              % (COMPRESSED_SOLVE_MS, PAIR_KERNEL_MS[0], PAIR_KERNEL_MS[1]), "",
              "| rel_tol | rtol | steps | products | solves | largest residual before / after | converged | host | products | solves | Krylov kernels | variances | compressed variances | largest gap |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for f in r["fits"]:
        c = f["variance_compressed"]
        for q in f["variance_exact"]:
            lines.append("| %g | %g | %d | %d | %d | %.3g / %.3g | %s | %.0f ms | %.0f ms | %.1f ms | %.1f ms | [%.3g, %.3g] | [%.3g, %.3g] (%.0f ms) | %.3g |"
                         % (f["rel_tol"], q["rtol"], q["iterations"], q["products"], q["solves"], q["residual0"], q["residual_max"],
                            "yes" if q["converged"] else "no", q["host_ms"], q["ms"]["product_ms"], q["ms"]["solve_ms"], q["ms"]["krylov_ms"],
                            q["min"], q["max"], c["min"], c["max"], c["host_ms"], q["gap"]))
    lines += ["", "## The Krylov kernels' share of a step", "",
              "`hssk_krylov_orth` (four launches and three `hssk_sum_slabs`) against `hssk_kernel_matmul` with the same columns, device events,",
              "mean of %d calls.  Bytes asked for, per row and column 8 x (4 (k + 1) + 7): the k + 1 blocks four times (the dots once, the" % r["kernel_reps"],
              "first update twice -- to update and for the dots of the new w --, the second update once), w read by each of the four launches",
              "and written by both updates, block k + 1 written by the finish.", "",
              "| nc | k | orth | product | share of orth + product | bytes moved | rate |", "|---|---|---|---|---|---|---|"]
    for q in r["kernels"]:
        lines.append("| %d | %d | %.3f ms | %.2f ms | %.1f %% | %.3f GB | %.2f TB/s |"
                     % (q["nc"], q["k"], q["orth_ms"], q["product_ms"], 100 * q["share"], q["gbytes"], q["tb_per_s"]))
    lines += ["", "The rate is bytes asked for over time, not HBM traffic: in the first update a thread reads its entry of every block to",
              "update w and again for the dots of the new w, so a quarter of the reads of the blocks find their line in the caches, and",
              "a rate above what HBM delivers says no more than that.  A single column is seven launches of 391 workgroups over a few",
              "megabytes: launch-bound, and next to the product it does not matter.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--leaf", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--render", default=None, help="write --md from the JSON line of an earlier run (--out) and measure nothing")
    a = ap.parse_args()
    if a.render:
        with open(a.render) as f, open(a.md, "w") as g:
            g.write(markdown(json.loads(f.readline())))
        return
    import torch
    assert torch.cuda.is_available(), "gp_refine_bench.py measures on the GPU"
    from strumpack_amd import _loader
    from strumpack_amd import kernel as KM
    lib = KM.load(_loader.lib_path())
    rng = np.random.default_rng(2025)
    X = rng.random((a.n, 8))
    y = np.sign((X - 0.5) @ rng.standard_normal(8))
    h, lam = 1.3, 3.11
    res = {"n": a.n, "leaf": a.leaf, "h": h, "lambda": lam, "kernel_reps": a.reps, "fits": []}
    for rel_tol in (1e-2, 1e-4):
        res["fits"].append(refine_runs(KM, lib, X, y, h, lam, a.leaf, rel_tol, (1e-6, 1e-8)))
        print(json.dumps(res["fits"][-1]), flush=True)
    res["kernels"] = kernel_runs(a.n, a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))


if __name__ == "__main__":
    main()
