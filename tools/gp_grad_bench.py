"""What the gradient of the log marginal likelihood costs next to the fit and the set_lambda step it steers
(profiles/gp_gradient.md).

One process, the workload of tools/gp_bench.py: N points uniform in [0, 1)^8, Gauss kernel h = 1.3, lambda = 3.11, cobble
clustering, leaf 128, rel_tol 1e-2, 64 neighbours.  Needs the GPU (the product library; no fallback).

  fit            STRUMPACK_kernel_fit_HSS_double with keep_model: host clock around the call (third fit of the process)
  set_lambda     SPX_kernel_model_set_lambda, alternating between two values: host clock
  gradient       SPX_kernel_lml_gradient with 63 probes (one block of 64 columns with alpha) and with 127 (two blocks): host
                 clock, and the device-event split of the call into kernel products, solves and column dot products
                 (SPX_kernel_gradient_ms), per block of 64 columns
  product        from the split: 2 n^2 64 flops of one block against the FP64 matrix-core roof, and n^2 exponentials per second
  residual       SPX_kernel_model_residual (one product with a single column): host clock

    python tools/gp_grad_bench.py --n 100000 --out gp_grad_bench.json --md gp_gradient.md
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MFMA_TFLOPS = 78.6          # gfx950 FP64 matrix peak (strumpack_amd/csrc/kernels/hssk_dgemm.hip)
CROSS_CHUNK_MS = 54.0            # one hssk_kernel_cross chunk of 64 x 1e5 pairs on a single workgroup (profiles/gp_variance.md)
PARENT_FIT_MS, PARENT_SET_LAMBDA_MS = 22.2, 3.0   # the parent commit's figures (profiles/gp_variance.md)


def clock(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": min(ts), "median_ms": float(np.median(ts)), "first_ms": ts[0], "reps": reps}


def gradient_runs(kr, probes, reps):
    walls, splits, val = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        val = kr.log_marginal_likelihood_gradient(probes=probes, seed=1, terms=True)
        walls.append((time.perf_counter() - t0) * 1e3)
        splits.append(kr.gradient_ms())
    blocks = (probes + 1 + 63) // 64
    best = splits[int(np.argmin(walls))]
    t = val[2]
    se = lambda v: float(np.std(v, ddof=1) / np.sqrt(len(v))) if len(v) > 1 else float("nan")
    return {"probes": probes, "blocks": blocks, "host_ms": walls, "device_ms": splits,
            "per_block_ms": {k: v / blocks for k, v in best.items()}, "dh": val[0], "dlambda": val[1],
            "quad_h": float(t["quad_h"]), "quad_lambda": float(t["quad_lambda"]), "trace_h": float(t["trace_h"]),
            "trace_lambda": float(t["trace_lambda"]), "trace_h_se": se(t["th"]), "trace_lambda_se": se(t["tl"])}


def markdown(r):
    g, g2, n = r["gradient63"], r["gradient127"], r["n"]
    pb = g["per_block_ms"]
    prod_s = pb["product_ms"] / 1e3
    tf = 2.0 * n * n * 64 / prod_s / 1e12
    exps = n * n / prod_s
    fit, sl, gh = r["fit"]["host_ms"][-1], r["set_lambda"]["min_ms"], min(g["host_ms"])
    chunks = (n + 63) // 64
    lines = [
        "# Gradient of the log marginal likelihood from the kept fit",
        "",
        "Tool: `tools/gp_grad_bench.py` (one process; the workload of `tools/gp_bench.py`: N = %d points uniform in [0, 1)^8, Gauss," % n,
        "h = 1.3, lambda = 3.11, cobble, leaf %d, rel_tol 1e-2, 64 neighbours).  Host clocks around calls that end in a device" % r["leaf"],
        "synchronise; the split of a gradient call comes from device events around the launches of each block of 64 columns.",
        "",
        "## Times on the MI355X",
        "",
        "| quantity | time | next to |",
        "|---|---|---|",
        "| fit with `keep_model` (host clock, third fit) | %.1f ms | parent commit: %.1f ms |" % (fit, PARENT_FIT_MS),
        "| `set_lambda` (minimum of %d) | %.2f ms | parent commit: %.1f ms |" % (r["set_lambda"]["reps"], sl, PARENT_SET_LAMBDA_MS),
        "| gradient, 63 probes = one block with alpha (host clock, minimum of %d) | %.1f ms | %.2f x the fit, %.1f x `set_lambda` |"
        % (len(g["host_ms"]), gh, gh / fit, gh / sl),
        "| - kernel product `hssk_kernel_matmul`, per block (device events) | %.2f ms | |" % pb["product_ms"],
        "| - solve in place, per block | %.3f ms | |" % pb["solve_ms"],
        "| - column dot products, per block | %.3f ms | |" % pb["dots_ms"],
        "| gradient, 127 probes = two blocks (host clock) | %.1f ms | per block: product %.2f, solve %.3f, dots %.3f ms |"
        % (min(g2["host_ms"]), g2["per_block_ms"]["product_ms"], g2["per_block_ms"]["solve_ms"], g2["per_block_ms"]["dots_ms"]),
        "| `fit_residual` (one product with one column, host clock) | %.1f ms | value %.4g |" % (r["residual"]["min_ms"], r["residual"]["value"]),
        "",
        "## The product kernel",
        "",
        "One block is n^2 = %.3g kernel evaluations and 2 n^2 64 = %.3g flops on the matrix cores." % (float(n) * n, 2.0 * n * n * 64),
        "",
        "- %.2f TFLOP/s on `v_mfma_f64_16x16x4_f64`: %.1f %% of the %.1f TFLOP/s FP64 matrix roof." % (tf, 100 * tf / FP64_MFMA_TFLOPS, FP64_MFMA_TFLOPS),
        "- %.3g `exp` evaluations per second (each with its %d FP64 coordinate differences)." % (exps, 8),
        "- The single-workgroup route would be %d chunks of `hssk_kernel_cross` at %.0f ms each, %.0f s: the product costs %.2g of that."
        % (chunks, CROSS_CHUNK_MS, chunks * CROSS_CHUNK_MS / 1e3, pb["product_ms"] / (chunks * CROSS_CHUNK_MS)),
        "",
        "## Values",
        "",
        "dL/dh = %.6g, dL/dlambda = %.6g with 63 probes (quad_h %.6g, trace_h %.6g +- %.3g; quad_lambda %.6g, trace_lambda %.6g +- %.3g:"
        % (g["dh"], g["dlambda"], g["quad_h"], g["trace_h"], g["trace_h_se"], g["quad_lambda"], g["trace_lambda"], g["trace_lambda_se"]),
        "the standard errors of the Hutchinson means from the per-probe values).  With 127 probes: dL/dh = %.6g, dL/dlambda = %.6g." % (g2["dh"], g2["dlambda"]),
        "These are gradients of the exact-kernel likelihood evaluated with the inverse of the matrix compressed at rel_tol 1e-2",
        "(DESIGN 8d): `fit_residual` above says how far that matrix is from the exact one.",
        "",
    ]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--leaf", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "gp_grad_bench.py measures on the GPU"
    from strumpack_amd import _loader
    from strumpack_amd import kernel as KM
    lib = KM.load(_loader.lib_path())
    rng = np.random.default_rng(2025)
    X = rng.random((a.n, 8))
    y = np.sign((X - 0.5) @ rng.standard_normal(8))
    h, lam, lam2 = 1.3, 3.11, 1.0
    argv = ["--hss_leaf_size", str(a.leaf), "--hss_rel_tol", "1e-2", "--hss_abs_tol", "1e-8", "--hss_approximate_neighbors", "64"]
    res = {"n": a.n, "leaf": a.leaf, "h": h, "lambda": lam}
    kr = KM.KernelRegression(lib, h=h, lam=lam, kernel="rbf", argv=argv, keep_model=True)
    fits = []
    for _ in range(3):                              # (the first fit of a process loads code objects and fills the device pool)
        t0 = time.perf_counter()
        kr.fit(X, y)
        fits.append((time.perf_counter() - t0) * 1e3)
    res["fit"] = {"host_ms": fits}
    res["log_marginal_likelihood"] = kr.log_marginal_likelihood()
    flip = [lam2, lam]
    res["set_lambda"] = clock(lambda: kr.set_lambda(flip[0]) and flip.reverse(), 2 * a.reps)
    if kr.lam != lam:
        kr.set_lambda(lam)
    res["gradient63"] = gradient_runs(kr, 63, a.reps)
    res["gradient127"] = gradient_runs(kr, 127, max(2, a.reps // 2))
    res["residual"] = dict(clock(kr.fit_residual, 3), value=kr.fit_residual())
    kr.destroy()
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
