"""Mixed-precision exact solves against the FP64 ones, in the same run (profiles/gp_mixed.md).

One process, the workload of tools/gp_refine_bench.py: N points uniform in [0, 1)^8, Gauss kernel h = 1.3, lambda = 3.11, cobble
clustering, leaf 128, 64 neighbours.  Needs the GPU (the product library; no fallback) -- except `--sections sweep --lib PATH`,
which runs the inner_rtol sweep alone on any build of the library (the CPU emulator at a small N).

  kernels    hssk_kernel_matmul_f32 against hssk_kernel_matmul with the same columns (device events, mean of --reps calls after
             an untimed one) at N and at 32768, nc = 1 and 64; the FP32 product's share of the FP32 matrix roof (157 TFLOP/s)
             from the flops the ALGORITHM needs -- 2 N^2 nc for g B, 2 N^2 (d + 2) for the exponents of matrix-core tiles; the
             32 or 64 columns the matrix cores are issued for a narrower block are not counted -- and its exp rate (N^2 per call)
  refine     KernelRegression.refine from the rel_tol 1e-4 and 1e-2 fits to rtol 1e-6 and 1e-8 in both modes, each from the
             compressed weights: steps, cycles, FP64 and FP32 products, host clock, device-event split
  variance   one chunk of 64 test points through predict_variance(exact=True) in both modes
  sweep      cycles and FP64 products to rtol 1e-8 for inner_rtol in {1e-2, 1e-3, 1e-4, 1e-5, off (1e-300)}

    python tools/gp_mixed_bench.py --n 100000 --out gp_mixed_bench.json --md gp_mixed.md [--emu emu_sweep.json]
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

ROOF_TFLOPS = 157.0
INNER_RTOLS = (1e-2, 1e-3, 1e-4, 1e-5, 1e-300)


def workload(n):
    rng = np.random.default_rng(2025)
    X = rng.random((n, 8))
    y = np.sign((X - 0.5) @ rng.standard_normal(8))
    return X, y, 1.3, 3.11


def fit(KM, lib, X, y, h, lam, leaf, rel_tol):
    argv = ["--hss_leaf_size", str(leaf), "--hss_rel_tol", "%g" % rel_tol, "--hss_abs_tol", "1e-8", "--hss_approximate_neighbors", "64"]
    kr = KM.KernelRegression(lib, h=h, lam=lam, kernel="rbf", argv=argv, keep_model=True)
    t0 = time.perf_counter()
    kr.fit(X, y)
    return kr, (time.perf_counter() - t0) * 1e3


def one_refine(kr, lam, rtol, inner, inner_rtol=None, maxit=100):
    kr.set_lambda(lam)                          # the compressed weights again
    t0 = time.perf_counter()
    info = kr.refine(rtol=rtol, maxit=maxit, inner=inner, inner_rtol=inner_rtol)
    wall = (time.perf_counter() - t0) * 1e3
    st = np.zeros(6)
    kr.L.SPX_kernel_krylov_stats(kr.K, st.ctypes.data)
    return dict(rtol=rtol, inner=inner, inner_rtol=inner_rtol, host_ms=wall, ms=kr.krylov_ms(), ms64=st[4], ms32=st[5], converged=info["converged"],
                iterations=info["iterations"], products=info["products"], products32=info["products32"], fallbacks=info["fallbacks"],
                solves=info["solves"], cycles=info["cycles"], residual0=info["residual0"], residual=info["residual"])


def refine_runs(KM, lib, X, y, h, lam, leaf, rel_tol, rtols, variance=True):
    kr, _ = fit(KM, lib, X, y, h, lam, leaf, rel_tol)
    t0 = time.perf_counter()
    kr.fit(X, y)                                    # (the first fits of a process load code objects and fill the device pool)
    fit_ms = (time.perf_counter() - t0) * 1e3
    out = {"rel_tol": rel_tol, "fit_ms": fit_ms, "fit_residual": kr.fit_residual(), "runs": [], "variance": []}
    one_refine(kr, lam, 1e-2, "f32", maxit=3)       # (untimed: the FP32 kernels' code objects)
    for rtol in rtols:
        for inner in ("f64", "f32"):
            out["runs"].append(one_refine(kr, lam, rtol, inner))
    if variance:
        T = np.random.default_rng(7).random((64, X.shape[1]))
        kr.set_lambda(lam)
        for inner in ("f64", "f32"):
            t0 = time.perf_counter()
            ve, info = kr.predict_variance(T, exact=True, rtol=1e-8, info=True, inner=inner)
            st = np.zeros(6)
            kr.L.SPX_kernel_krylov_stats(kr.K, st.ctypes.data)
            out["variance"].append(dict(inner=inner, host_ms=(time.perf_counter() - t0) * 1e3, ms64=st[4], ms32=st[5], converged=info["converged"],
                                        iterations=info["iterations"], products=info["products"], products32=info["products32"],
                                        fallbacks=info["fallbacks"], cycles=info["cycles"], residual_max=info["residual_max"],
                                        min=float(ve.min()), max=float(ve.max())))
    kr.destroy()
    return out


def sweep_runs(KM, lib, X, y, h, lam, leaf, rel_tols):
    out = []
    for rel_tol in rel_tols:
        kr, _ = fit(KM, lib, X, y, h, lam, leaf, rel_tol)
        base = one_refine(kr, lam, 1e-8, "f64")
        rows = [one_refine(kr, lam, 1e-8, "f32", irt) for irt in INNER_RTOLS]
        out.append(dict(rel_tol=rel_tol, n=len(X), f64=base, rows=rows))
        kr.destroy()
    return out


def kernel_runs(path, sizes, reps):
    from strumpack_amd import hssk as K
    hk = K.Hssk(path)
    L = hk.lib
    L.hssk_watch_start.argtypes = L.hssk_watch_stop.argtypes = [C.c_void_p, C.c_int]
    L.hssk_watch_read_ms.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.hssk_watch_read_ms.restype = C.c_double
    d, res = 8, []
    for n in sizes:
        dX = hk.array(np.random.default_rng(1).random((d, n)))
        spec = K.KernelSpec(dX.ptr, n, d, 0, 1, 1.3, 3.11)
        nb = L.hssk_kernel_matmul_f32_prep_bytes(n, d)
        dP = hk.empty((nb,), np.uint8)
        L.hssk_watch_start(hk.ctx, 3)
        hk.check(L.hssk_kernel_matmul_f32_prep(hk.ctx, C.byref(spec), dP.ptr, nb))
        L.hssk_watch_stop(hk.ctx, 3)
        prep_ms = L.hssk_watch_read_ms(hk.ctx, 3, None)
        for nc in (1, 64):
            dW, dO, dQ = hk.empty((n, nc)), hk.empty((n, nc)), hk.empty((n, nc))
            hk.check(L.hssk_randn(hk.ctx, dW.ptr, n, nc, n, 0, nc, 9))
            st = np.zeros(4, dtype=np.int64)
            for timed in (False, True):             # (one untimed call of each first)
                for _ in range(reps if timed else 1):
                    L.hssk_watch_start(hk.ctx, 1)
                    hk.check(L.hssk_kernel_matmul_f32(hk.ctx, C.byref(spec), dP.ptr, dW.ptr, n, nc, dQ.ptr, n, 0, None))
                    L.hssk_watch_stop(hk.ctx, 1)
                    L.hssk_watch_start(hk.ctx, 2)
                    hk.check(L.hssk_kernel_matmul(hk.ctx, C.byref(spec), 0, dW.ptr, n, nc, dO.ptr, n, 0))
                    L.hssk_watch_stop(hk.ctx, 2)
                f32, f64 = L.hssk_watch_read_ms(hk.ctx, 1, None) / reps, L.hssk_watch_read_ms(hk.ctx, 2, None) / reps
            hk.check(L.hssk_kernel_matmul_f32(hk.ctx, C.byref(spec), dP.ptr, dW.ptr, n, nc, dQ.ptr, n, 0, st.ctypes.data))
            a, b = dO.get(), dQ.get()
            tiles = max(1, int(st[0] + st[1]))
            flops = 2.0 * n * n * nc + 2.0 * n * n * (d + 2) * st[0] / tiles    # (what the algorithm needs, not the padded columns)
            res.append(dict(n=n, nc=nc, f32_ms=f32, f64_ms=f64, prep_ms=prep_ms, mfma_tiles=int(st[0]), diff_tiles=int(st[1]), splits=int(st[2]),
                            tflops=flops / (f32 * 1e-3) / 1e12, roof_share=flops / (f32 * 1e-3) / 1e12 / ROOF_TFLOPS, gexp_per_s=n * float(n) / (f32 * 1e-3) / 1e9,
                            rel_diff=float(np.abs(a - b).max() / np.abs(a).max())))
            for v in (dW, dO, dQ):
                v.free()
        dX.free()
        dP.free()
    hk.close()
    return res


def beat(a, b):
    return "yes" if a < b else "NO"


def markdown(r, emu=None):
    n = r["n"]
    L = ["# Mixed-precision exact solves: FP32 matrix-core product inside GMRES",
         "",
         "Tool: `tools/gp_mixed_bench.py` (one process; the workload of `tools/gp_refine_bench.py`: N = %d points uniform in [0, 1)^8, Gauss," % n,
         "h = 1.3, lambda = 3.11, cobble, leaf %d, 64 neighbours).  Every mixed figure stands next to the FP64 figure of the SAME run." % r["leaf"],
         "Host clocks around calls that end in a device synchronise; kernel times from device events.  Defaults: maxit 100, restart 30,",
         "inner_rtol 1e-4.", ""]
    if r.get("kernels"):
        L += ["## The product: `hssk_kernel_matmul_f32` against `hssk_kernel_matmul`", "",
              "Same columns, device events, mean of %d calls after an untimed one.  Flops: what the algorithm needs, 2 N^2 nc for the product" % r["reps"],
              "plus 2 N^2 (d + 2) for the exponents of matrix-core tiles (not the 32 or 64 columns the matrix cores are issued for); roof",
              "157 TFLOP/s.  exp rate: N^2 kernel values per call.", "",
              "| N | nc | FP64 product | FP32 product | FP32 faster | speed-up | prep (once per call of the solver) | tiles matrix cores / difference | splits | TFLOP/s | share of the FP32 roof | exp rate | largest difference / largest entry |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for q in r["kernels"]:
            L.append("| %d | %d | %.2f ms | %.2f ms | %s | %.1f x | %.3f ms | %d / %d | %d | %.1f | %.1f %% | %.0f G/s | %.2g |"
                     % (q["n"], q["nc"], q["f64_ms"], q["f32_ms"], beat(q["f32_ms"], q["f64_ms"]), q["f64_ms"] / q["f32_ms"], q["prep_ms"], q["mfma_tiles"],
                        q["diff_tiles"], q["splits"], q["tflops"], 100 * q["roof_share"], q["gexp_per_s"], q["rel_diff"]))
        L.append("")
    if r.get("fits"):
        L += ["## refine", "",
              "| rel_tol | fit | residual before | rtol | mode | steps | cycles | FP64 products | FP32 products | fallbacks | residual after | converged | host | FP64 products | FP32 products | solves | Krylov kernels | mixed beat FP64 |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for f in r["fits"]:
            for a, b in zip(f["runs"][0::2], f["runs"][1::2]):
                for q in (a, b):
                    L.append("| %g | %.0f ms | %.3g | %g | %s | %d | %d | %d | %d | %d | %.3g | %s | %.0f ms | %.0f ms | %.0f ms | %.1f ms | %.1f ms | %s |"
                             % (f["rel_tol"], f["fit_ms"], q["residual0"], q["rtol"], q["inner"], q["iterations"], q["cycles"], q["products"], q["products32"],
                                q["fallbacks"], q["residual"], "yes" if q["converged"] else "no", q["host_ms"], q["ms64"], q["ms32"], q["ms"]["solve_ms"],
                                q["ms"]["krylov_ms"], "" if q is a else ("%s (%.2f x)" % (beat(b["host_ms"], a["host_ms"]), a["host_ms"] / b["host_ms"]))))
        L.append("")
        for f in r["fits"]:
            for a, b in zip(f["runs"][0::2], f["runs"][1::2]):
                verdict = ("mixed beat FP64: %.0f ms against %.0f ms" if b["host_ms"] < a["host_ms"] else "mixed did NOT beat FP64: %.0f ms against %.0f ms") % (b["host_ms"], a["host_ms"])
                L.append("- rel_tol %g, rtol %g: %s; FP64 %s (residual %.3g), mixed %s (residual %.3g)."
                         % (f["rel_tol"], a["rtol"], verdict, "converged" if a["converged"] else "did not converge in %d steps" % a["iterations"], a["residual"],
                            "converged" if b["converged"] else "did not converge in %d steps" % b["iterations"], b["residual"]))
        L += ["", "## One exact variance chunk of 64 test points (rtol 1e-8)", "",
              "| rel_tol | mode | steps | cycles | FP64 products | FP32 products | fallbacks | largest residual after | converged | host | FP64 products | FP32 products | variances | mixed beat FP64 |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for f in r["fits"]:
            if not f["variance"]:
                continue
            a, b = f["variance"]
            for q in (a, b):
                L.append("| %g | %s | %d | %d | %d | %d | %d | %.3g | %s | %.0f ms | %.0f ms | %.0f ms | [%.3g, %.3g] | %s |"
                         % (f["rel_tol"], q["inner"], q["iterations"], q["cycles"], q["products"], q["products32"], q["fallbacks"], q["residual_max"],
                            "yes" if q["converged"] else "no", q["host_ms"], q["ms64"], q["ms32"], q["min"], q["max"],
                            "" if q is a else ("%s (%.2f x)" % (beat(b["host_ms"], a["host_ms"]), a["host_ms"] / b["host_ms"]))))
        L.append("")
    for title, sw in (("## inner_rtol on the N = %d workload (rtol 1e-8)" % n, r.get("sweep")),
                      ("## inner_rtol on the CPU emulator (rtol 1e-8)", emu)):
        if not sw:
            continue
        L += [title, "", "| N | rel_tol | mode | inner_rtol | steps | cycles | FP64 products | FP32 products | fallbacks | converged | residual after | host |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for s in sw:
            for q in [s["f64"]] + s["rows"]:
                irt = "" if q["inner"] == "f64" else ("off" if q["inner_rtol"] < 1e-100 else "%g" % q["inner_rtol"])
                L.append("| %d | %g | %s | %s | %d | %d | %d | %d | %d | %s | %.3g | %.0f ms |"
                         % (s["n"], s["rel_tol"], q["inner"], irt, q["iterations"], q["cycles"], q["products"], q["products32"], q["fallbacks"],
                            "yes" if q["converged"] else "no", q["residual"], q["host_ms"]))
        L.append("")
    tables = [s for sw in (r.get("sweep"), emu) if sw for s in sw if any(q["converged"] for q in s["rows"])]
    if tables:
        L += ["## The default inner_rtol", "", "Per table with a converged mixed run: the fewest FP64 products and the values that reach them.", ""]
        best_everywhere = None
        for s in tables:
            conv = [q for q in s["rows"] if q["converged"]]
            fewest = min(q["products"] for q in conv)
            vals = [q["inner_rtol"] for q in conv if q["products"] == fewest]
            best_everywhere = set(vals) if best_everywhere is None else best_everywhere & set(vals)
            L.append("- N = %d, rel_tol %g: %d FP64 products (FP64 mode: %d) at inner_rtol %s."
                     % (s["n"], s["rel_tol"], fewest, s["f64"]["products"], ", ".join("off" if v < 1e-100 else "%g" % v for v in vals)))
        keep = sorted(v for v in (best_everywhere or ()) if v > 1e-100)
        L += ["", "The loosest value that reaches the minimum in every table: %s.  The library's default is 1e-4 (`KRYLOV_INNER_RTOL_DEFAULT`)."
              % ("%g" % keep[-1] if keep else "none"), ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--leaf", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sections", default="kernels,refine,sweep")
    ap.add_argument("--lib", default=None, help="library to load (default: the product library)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--emu", default=None, help="JSON of an earlier `--sections sweep --lib <emulator>` run to print next to the GPU sweep")
    ap.add_argument("--render", default=None, help="write --md from the JSON line of an earlier run (--out) and measure nothing")
    a = ap.parse_args()
    emu = None
    if a.emu:
        with open(a.emu) as f:
            emu = json.loads(f.readline())["sweep"]
    if a.render:
        with open(a.render) as f, open(a.md, "w") as g:
            g.write(markdown(json.loads(f.readline()), emu))
        return
    from strumpack_amd import _loader
    from strumpack_amd import kernel as KM
    path = a.lib or _loader.lib_path()
    if not a.lib:
        import torch
        assert torch.cuda.is_available(), "gp_mixed_bench.py measures on the GPU"
    lib = KM.load(path)
    sections = a.sections.split(",")
    X, y, h, lam = workload(a.n)
    res = {"n": a.n, "leaf": a.leaf, "h": h, "lambda": lam, "reps": a.reps}
    if "kernels" in sections:
        res["kernels"] = kernel_runs(path, sorted({a.n, min(a.n, 32768)}, reverse=True), a.reps)
        print(json.dumps(res["kernels"]), flush=True)
    if "refine" in sections:
        res["fits"] = []
        for rel_tol in (1e-4, 1e-2):
            res["fits"].append(refine_runs(KM, lib, X, y, h, lam, a.leaf, rel_tol, (1e-6, 1e-8)))
            print(json.dumps(res["fits"][-1]), flush=True)
    if "sweep" in sections:
        res["sweep"] = sweep_runs(KM, lib, X, y, h, lam, a.leaf, (1e-4, 1e-2))
        print(json.dumps(res["sweep"]), flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res, emu))


if __name__ == "__main__":
    main()
