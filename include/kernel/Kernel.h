/* C interface to kernel ridge regression through an HSS approximation of the kernel matrix, computed on the
 * MI355X.  Same entry points as the reference's src/kernel/Kernel.h:43-80 (double precision; the reference's
 * Python wrapper src/python/STRUMPACKKernel.py.in binds exactly these through ctypes).
 *
 *   STRUMPACK_create_kernel_double   Kernel.h:43   train: d x n, one point per column (copied);
 *                                                  type 0 Gauss, 1 Laplace, 2 ANOVA (degree p)
 *   STRUMPACK_kernel_fit_HSS_double  Kernel.h:51   argv carries --hss_* options (default clustering: cobble,
 *                                                  Kernel.cpp:81-83); labels: n values
 *   STRUMPACK_kernel_predict_double  Kernel.h:77   test: d x m; prediction: m values out
 *   STRUMPACK_destroy_kernel_double  Kernel.h:48
 */
#ifndef STRUMPACK_C_KERNEL_HPP
#define STRUMPACK_C_KERNEL_HPP

typedef void* STRUMPACKKernel;

#ifdef __cplusplus
extern "C" {
#endif

STRUMPACKKernel STRUMPACK_create_kernel_double(int n, int d, double* train, double h, double lambda, int p, int type);
void STRUMPACK_destroy_kernel_double(STRUMPACKKernel K);
void STRUMPACK_kernel_fit_HSS_double(STRUMPACKKernel K, double* labels, int argc, char* argv[]);
void STRUMPACK_kernel_predict_double(STRUMPACKKernel K, int m, double* test, double* prediction);

/* Single precision, the reference's src/kernel/Kernel.h:45-80 (its Python estimator binds these for float32 data).  The fit is
 * promoted: points and labels are widened exactly, the FP64 front end runs, the weights are rounded once to float; train and
 * labels are reordered into cluster order in place.  Prediction is native FP32 on the device, from a model that stays in HBM
 * between calls.  The SPX_ introspection calls below take either kind of handle. */
STRUMPACKKernel STRUMPACK_create_kernel_float(int n, int d, float* train, float h, float lambda, int p, int type);
void STRUMPACK_destroy_kernel_float(STRUMPACKKernel K);
void STRUMPACK_kernel_fit_HSS_float(STRUMPACKKernel K, float* labels, int argc, char* argv[]);
void STRUMPACK_kernel_predict_float(STRUMPACKKernel K, int m, float* test, float* prediction);
/* the same prediction with test points (d x m, one point per column) and predictions (m) already in HBM, e.g. a torch tensor: no
 * host copy of either; the work enqueued on the caller's stream must have finished, the result is complete on return.
 * Non-zero: a pointer that is not a device pointer, no fit, or a double handle */
int SPX_kernel_predict_device_float(STRUMPACKKernel K, int m, const float* dtest, float* dpred);
/* the last float prediction of the handle: out[0] tiles (64 x 64 pairs) taken on the matrix cores, [1] tiles taken in the
 * difference form, [2] splits of the training set, [3] device-clock microseconds of the prediction launches, [4] bytes uploaded
 * by the call, [5] 1 if the model was already resident */
int SPX_kernel_predict_stats(STRUMPACKKernel K, long long* out);

/* ---- extensions (SPX_): introspection for tests / benchmarks --------------------------------------------- */
/* after fit: out[0] compressed (0/1), [1] levels, [2] max rank, [3] memory bytes, [4] neighbour count used,
 * [5] compress us, [6] factor us, [7] solve us */
int SPX_kernel_fit_info(STRUMPACKKernel K, long long* out);
/* pre-order node table of the last fit, 6 ints per node (row_offset, rows, U_rows, U_rank, V_rank, is_leaf);
 * returns the node count */
int SPX_kernel_node_info(STRUMPACKKernel K, int* out, int cap);
/* tests: neighbour lists (k x n ints, 0-based ids in CLUSTER order, column i = point i) used instead of the device
 * search in the first compression round of the next fit */
int SPX_kernel_set_neighbors(STRUMPACKKernel K, int k, const int* ann);
/* the 1-based permutation of the training points chosen by the clustering (n ints) and the weights (n doubles,
 * in permuted order) */
int SPX_kernel_permutation(STRUMPACKKernel K, int* perm);
int SPX_kernel_weights(STRUMPACKKernel K, double* w);
/* ---- the kept model: log-determinant, log marginal likelihood, predictive variance, a new lambda without a new compression.
 * Double handles with a built-in kernel.  SPX_kernel_keep_model(K, 1) before the fit makes STRUMPACK_kernel_fit_HSS_double keep the
 * factored HSS matrix, the cluster-ordered points in HBM, the permuted labels and the weights until the next fit,
 * SPX_kernel_keep_model(K, 0) or the destroy call; without it the fit keeps nothing, as before.  Every call below returns
 * non-zero, its outputs untouched, without a kept model, on a float handle and for a user-defined kernel. */
int SPX_kernel_keep_model(STRUMPACKKernel K, int keep);
/* *out = log|det H|, H the compressed K + lambda I (read off the ULV factors) */
int SPX_kernel_logabsdet(STRUMPACKKernel K, double* out);
/* *out = -1/2 y^T alpha - 1/2 log|det H| - n/2 log(2 pi)   (y: the permuted labels, alpha: the weights) */
int SPX_kernel_log_marginal_likelihood(STRUMPACKKernel K, double* out);
/* var[c] = k(t_c, t_c) - k_c^T H^-1 k_c for the m test points (test: d x m): the variance of the latent function -- add lambda for
 * the observation noise.  Not clamped: H equals K + lambda I only up to the compression tolerance, so a value may be slightly
 * negative.  Works in chunks of 64 test points (cross-kernel block, device solve in place, column-weighted sum). */
int SPX_kernel_predict_variance_double(STRUMPACKKernel K, int m, const double* test, double* var);
/* device-clock milliseconds of the last variance call: out[0] cross-kernel blocks, [1] solves, [2] column sums */
int SPX_kernel_variance_ms(STRUMPACKKernel K, double* out);
/* a new lambda: shift(lambda - current), factor, solve of the kept labels.  The handle's weights and lambda are the new ones
 * afterwards (STRUMPACK_kernel_predict_double, SPX_kernel_weights and the calls above see them); ranks and tree are unchanged. */
int SPX_kernel_model_set_lambda(STRUMPACKKernel K, double lambda);
/* the kept matrix through HSSMatrix::write (layout: csrc/host/hss_io.cpp) */
int SPX_kernel_model_write(STRUMPACKKernel K, const char* path);
/* the kept labels (n doubles) and the training points (d x n), both in cluster order */
int SPX_kernel_model_labels(STRUMPACKKernel K, double* y);
int SPX_kernel_model_points(STRUMPACKKernel K, double* x);
/* The gradient of the log marginal likelihood L in the width h and in lambda (Gauss and Laplace):
 *   grad[0] = dL/dh = 1/2 alpha^T K' alpha - 1/2 tr(H^-1 K'),   grad[1] = dL/dlambda = 1/2 alpha^T alpha - 1/2 tr(H^-1),
 * K' = dK/dh the EXACT kernel derivative, H^-1 the kept, compressed and factored matrix, the traces estimated with the m >= 1
 * probe vectors z_k as the mean of s_k^T K' z_k and s_k^T z_k, s_k = H^-1 z_k.  Z: n x m column-major, rows in cluster order
 * (as SPX_kernel_model_points); NULL: the Rademacher block SPX_kernel_model_probes(m, seed) gives.  terms: NULL or 4 + 2 m
 * doubles: quad_h = 1/2 alpha^T K' alpha, quad_lambda = 1/2 alpha^T alpha, trace_h, trace_lambda (the means), then the m values
 * s_k^T K' z_k and the m values s_k^T z_k.  Non-zero also for an ANOVA kernel and for m < 1. */
int SPX_kernel_lml_gradient(STRUMPACKKernel K, int m, const double* Z, unsigned long long seed, double grad[2], double* terms);
/* The same gradient with one length scale per coordinate (automatic relevance determination; Gauss and Laplace, d <= 64;
 * DESIGN.md 8i): k_l(x, y) = k(x / l, y / l), theta_j = ln l_j taken at l = 1, i.e. on the points the model holds,
 *   grad[j] = dL/dtheta_j = 1/2 alpha^T K_j alpha - 1/2 tr(H^-1 K_j),   K_j = K o D_j,   sum_j grad[j] = h dL/dh,
 * D_j = (x_j - y_j)^2 / h^2 (Gauss), |x_j - y_j| / h (Laplace).  m, Z, seed as above.  grad: d doubles.  terms: NULL or
 * 2 d + d m doubles: the d values 1/2 alpha^T K_j alpha, the d trace means, then per coordinate the m values s_k^T K_j z_k.
 * A model fitted on X / w has dL/dw_j = grad[j] / w_j.  Non-zero, with the outputs untouched, without a kept model, for a float
 * handle, an ANOVA or Matern kernel, d > 64 and m < 1. */
int SPX_kernel_lml_gradient_coords(STRUMPACKKernel K, int m, const double* Z, unsigned long long seed, double* grad, double* terms);
/* the n x m block of +-1 entries the seeded form uses: std::mt19937_64(seed), one bit per entry, column by column */
int SPX_kernel_model_probes(STRUMPACKKernel K, int m, unsigned long long seed, double* Z);
/* *out = ||y - (K + lambda I) alpha||_2 / ||y||_2 with the EXACT kernel matrix: how far the compressed fit is from the exact one */
int SPX_kernel_model_residual(STRUMPACKKernel K, double* out);
/* device-clock milliseconds of the last gradient call: out[0] kernel products, [1] solves, [2] column dot products */
int SPX_kernel_gradient_ms(STRUMPACKKernel K, double* out);
/* ---- solves with the EXACT K + lambda I from the kept model (Gauss and Laplace): right-preconditioned restarted
 * GMRES on the device, the kept ULV factors as preconditioner, up to 64 columns in lockstep.  A column is converged when its true
 * residual ||b - (K + lambda I) x||_2 <= rtol ||b||_2; the steps of a call (per block of 64 columns) never exceed maxit; a cycle
 * has at most `restart` steps.  Not converging is NOT an error: the call returns 0 and info says so.  Non-zero, outputs
 * untouched and the model undisturbed: no kept model, a float handle, a user-defined or ANOVA kernel, rtol <= 0 or not finite,
 * maxit < 1, restart < 1, a leading dimension below n.
 * info: NULL or 8 + 2 m doubles (m the number of columns: 1 for the refine call, the test points for the variance):
 *   [0] converged (1 / 0: every column), [1] steps of the slowest column, [2] exact products, [3] ULV solves, [4] cycles (summed
 *   over the blocks), [5] largest relative residual at the start, [6] largest at the end, [7] m, then the m relative residuals
 *   at the end and the m step counts.
 * SPX_kernel_model_refine: the kept labels as right-hand side, the current weights as first iterate; the handle's weights become
 * the last iterate (SPX_kernel_weights, STRUMPACK_kernel_predict_double, SPX_kernel_model_residual and the y^T alpha of the log
 * marginal likelihood follow; SPX_kernel_logabsdet stays that of the compressed matrix).  SPX_kernel_model_set_lambda and a new
 * fit replace them by the compressed solve again. */
int SPX_kernel_model_refine(STRUMPACKKernel K, double rtol, int maxit, int restart, double* info);
/* X (n x m, ldx) = (K + lambda I)^-1 B (n x m, ldb), rows in cluster order, any m >= 0, from the first iterate H^-1 b; the model is
 * not changed */
int SPX_kernel_model_solve(STRUMPACKKernel K, int m, const double* B, int ldb, double* X, int ldx, double rtol, int maxit, int restart,
                           double* info);
/* SPX_kernel_predict_variance_double with the exact solve in place of the compressed one; not clamped */
int SPX_kernel_predict_variance_exact_double(STRUMPACKKernel K, int m, const double* test, double* var, double rtol, int maxit, int restart,
                                             double* info);
/* device-clock milliseconds of the last of these three calls: out[0] exact products, [1] ULV solves, [2] Krylov kernels (zeros
 * before the first one).  Refused like them: no kept model, a float handle, a user-defined or ANOVA kernel. */
int SPX_kernel_krylov_ms(STRUMPACKKernel K, double out[3]);
/* ---- mixed precision for the three calls above.  Handle state of a double handle with a built-in kernel, set like
 * SPX_kernel_keep_model (before or after the fit; a new lambda leaves it alone).  precision 0: FP64 (the default: every call is
 * what it was, bit for bit); 1: the product inside the restart cycles is the FP32 matrix-core product hssk_kernel_matmul_f32,
 * the true residual at every cycle's start -- where convergence is declared -- stays FP64.  inner_rtol: a column leaves its
 * cycle when the Arnoldi estimate is at most max(rtol ||b||, inner_rtol ||r at the cycle's start||); <= 0 takes the default
 * (1e-4), otherwise it must be below 1.  Non-zero and nothing changed: a float handle, an unknown precision, inner_rtol >= 1 or
 * not a number.  With precision 1 the three calls are also refused (model untouched) for more than 64 coordinates; ANOVA is
 * refused as before.  If a true residual does not decrease from one cycle start to the next, the rest of that block of columns
 * runs with the FP64 product: counted in the statistics, not an error. */
int SPX_kernel_set_krylov_inner(STRUMPACKKernel K, int precision, double inner_rtol);
int SPX_kernel_krylov_inner(STRUMPACKKernel K, int* precision, double* inner_rtol);
/* of the last of the three calls: out[0] FP64 products, [1] FP32 products, [2] fallbacks, [3] cycles, [4] ms of the FP64 products,
 * [5] ms of the FP32 products.  Refused like SPX_kernel_krylov_ms. */
int SPX_kernel_krylov_stats(STRUMPACKKernel K, double out[6]);
/* ---- gradients in the test points (double handles, Gauss and Laplace, d <= 64).  test: d x m, grad: d x m (one
 * gradient per column, in the coordinates of the points the handle was created with).  Every call returns non-zero, its outputs
 * untouched, for a float handle, an ANOVA or user-defined kernel, d > 64 and a handle that has not been fitted.
 * grad(j, c) = d prediction(t_c) / dt_cj = sum_r alpha_r dk(x_r, t_c) / dt_cj with the handle's weights: the gradient of
 * STRUMPACK_kernel_predict_double (a force, where the fit is an energy surface).  No kept model needed. */
int SPX_kernel_predict_gradient_double(STRUMPACKKernel K, int m, const double* test, double* grad);
/* SPX_kernel_predict_variance_double with grad(:, c) = -2 sum_r V(r, c) dk(x_r, t_c) / dt_c, V = H^-1 k(X, T) (d k(t, t) / dt = 0): var
 * is bit for bit what SPX_kernel_predict_variance_double returns.  grad is the derivative of var exactly when H is symmetric;
 * otherwise it is -2 D^T H^-1 k, D the derivative of k(X, t) in t.  Also refused without a kept model. */
int SPX_kernel_predict_variance_gradient_double(STRUMPACKKernel K, int m, const double* test, double* var, double* grad);
/* the same with the exact solve: var is bit for bit what SPX_kernel_predict_variance_exact_double returns; arguments, info and
 * refusals as there (SPX_kernel_set_krylov_inner is respected; the gradient sum itself is always FP64) */
int SPX_kernel_predict_variance_gradient_exact_double(STRUMPACKKernel K, int m, const double* test, double* var, double* grad, double rtol,
                                                      int maxit, int restart, double* info);
/* ---- the joint predictive covariance of the m test points: cov(a, b) = k(t_a, t_b) - (Q(a, b) + Q(b, a)) / 2,
 * Q = k(T, X) H^-1 k(X, T), column-major with ldc >= m; exactly symmetric, not clamped.  Its diagonal agrees with
 * SPX_kernel_predict_variance_double within rounding, not bit for bit (the sums run in another order).  Gauss and Laplace
 * fits, any d; non-zero, outputs untouched, without a kept model, for an ANOVA fit or a float handle. */
int SPX_kernel_predict_covariance_double(STRUMPACKKernel K, int m, const double* test, double* cov, int ldc);
/* the same with the exact solve; rtol, maxit, restart and info as for SPX_kernel_predict_variance_exact_double */
int SPX_kernel_predict_covariance_exact_double(STRUMPACKKernel K, int m, const double* test, double* cov, int ldc, double rtol, int maxit,
                                               int restart, double* info);
/* device-clock milliseconds of the last covariance call: ms3[0] cross-kernel blocks, [1] solves, [2] products */
int SPX_kernel_covariance_ms(STRUMPACKKernel K, double* ms3);
/* binary_tree_clustering on its own (clustering/Clustering.hpp:143-168): algo 0 natural, 1 2means, 2 kdtree,
 * 3 pca, 4 cobble; data (d x n) is reordered in place, perm is 1-based; returns the number of leaves and writes
 * at most cap leaf sizes */
int SPX_clustering(int n, int d, double* data, int algo, int leaf_size, int* perm, int* leaf_sizes, int cap);
/* the same with the median-split partitioners (2 kdtree, 4 cobble) on the device, one launch per tree level
 * (hssk_cluster_median); *status: 0 = done; > 0 = ties at a median / at the farthest point or a long displacement chain were
 * met, -1 = algorithm or dimension not taken by the device form -- data and perm are untouched then and the return value is 0
 * (SPX_clustering, the host form, decides such point sets).  This is what the kernel-matrix constructors call for point sets
 * of STRUMPACK_AMD_CLUSTER_DEVICE_MIN (default 8192) points and more, falling back to the host form on a non-zero status. */
int SPX_clustering_device(int n, int d, double* data, int algo, int leaf_size, int* perm, int* leaf_sizes, int cap, int* status);
/* find_approximate_neighbors on its own (clustering/NeighborSearch.cpp:324-345, host): ann / scores are k x n, column i =
 * the neighbours of point i, nearest first, the point itself included; scores (squared distances) may be NULL */
int SPX_approximate_neighbors(int n, int d, const double* data, int iterations, int k, int* ann, double* scores);

#ifdef __cplusplus
}
#endif
#endif
