// kernel::Kernel and its Gauss / Laplace / ANOVA subclasses (reference: kernel/Kernel.hpp:73-399,
// kernel/KernelRegression.hpp:56-123): a kernel matrix K(i, j) = k(x_i, x_j) + lambda [i == j] over the columns
// of a d x n point matrix, kernel ridge regression through an HSS approximation (fit_HSS) and prediction.
//
// The point set stays on the host in the caller's matrix (the reference keeps a reference to it and reorders
// it in place while clustering -- same here); entries needed by the HSS construction, the nearest-neighbour
// lists and the prediction sums are evaluated on the MI355X from a device copy (hssk_kernel_eval_vbatched,
// hssk_knn, hssk_kernel_predict).  eval() / operator() remain available on the host as the scalar API of the
// reference (single entries, small blocks); they are not on any compute path of this library.
#pragma once
#include <cmath>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "DenseMatrix.hpp"
#include "HSSOptions.hpp"

namespace strumpack {
namespace kernel {

enum class KernelType { DENSE, GAUSS, LAPLACE, ANOVA };

inline std::string get_name(KernelType k) {
  switch (k) {
    case KernelType::DENSE: return "dense";
    case KernelType::GAUSS: return "Gauss";
    case KernelType::LAPLACE: return "Laplace";
    case KernelType::ANOVA: return "ANOVA";
  }
  return "UNKNOWN";
}
inline KernelType kernel_type(const std::string& k) {
  if (k == "dense") return KernelType::DENSE;
  if (k == "Gauss") return KernelType::GAUSS;
  if (k == "Laplace") return KernelType::LAPLACE;
  if (k == "ANOVA") return KernelType::ANOVA;
  std::cerr << "ERROR: Kernel type not recogonized,  setting kernel type to Gauss." << std::endl;
  return KernelType::GAUSS;
}

template <typename scalar_t> class Kernel;

// what Kernel<double>::log_marginal_likelihood_gradient returns
struct LmlGradient {
  double dh = 0., dlambda = 0.;               // the gradient
  double quad_h = 0., quad_lambda = 0.;       // 1/2 alpha^T dK/dh alpha, 1/2 alpha^T alpha
  double trace_h = 0., trace_lambda = 0.;     // means of the per-probe values
  std::vector<double> th, tl;                 // per probe: s_k^T (dK/dh z_k), s_k^T z_k
};

// what Kernel<double>::log_marginal_likelihood_gradient_coords returns: the gradient in theta_j = ln l_j, one length scale l_j per
// coordinate, taken at l = 1
struct LmlGradientCoords {
  int m = 0;                                  // probes
  std::vector<double> dtheta, quad, trace;    // per coordinate: dL/dtheta_j = quad_j - trace_j / 2, 1/2 alpha^T K_j alpha, mean_k tc[j][k]
  std::vector<double> tc;                     // d x m, coordinate-major: tc[j m + k] = s_k^T (K_j z_k)
};

// what the solves with the EXACT kernel matrix report (Kernel<double>::model_refine / model_solve / predict_variance_exact)
struct KrylovInfo {
  bool converged = true;                        // every column reached rtol
  int iterations = 0;                           // steps of the slowest column
  long long products = 0, solves = 0, cycles = 0;   // exact products, ULV solves and restart cycles, summed over the blocks
  long long products32 = 0;                     // mixed mode: FP32 products inside the cycles (`products` then counts the FP64 ones alone)
  long long fallbacks = 0;                      // mixed mode: blocks whose true residual did not decrease and went on in FP64
  std::vector<int> its;                         // per column: steps it took part in
  std::vector<double> residual, residual0;      // per column: ||b - (K + lambda I) x|| / ||b|| at the end and at the start (true ones)
  double ms[4] = {0., 0., 0., 0.};              // device-clock milliseconds: FP64 products, solves, Krylov kernels, FP32 products
};

// the precision of the product INSIDE the cycles of the exact solves (Kernel<double>::krylov_inner)
enum class KrylovInner { FP64, FP32 };
constexpr double KRYLOV_INNER_RTOL_DEFAULT = 1e-4;

template <> class Kernel<double> {
  using scalar_t = double;
  using DenseM_t = DenseMatrix<double>;

 public:
  Kernel(DenseM_t& data, scalar_t lambda);
  virtual ~Kernel();
  Kernel(const Kernel&) = delete;
  Kernel& operator=(const Kernel&) = delete;

  std::size_t n() const { return data_.cols(); }
  std::size_t d() const { return data_.rows(); }

  virtual scalar_t eval(std::size_t i, std::size_t j) const {
    return eval_kernel_function(data_.ptr(0, i), data_.ptr(0, j)) + ((i == j) ? lambda_ : scalar_t(0.));
  }
  void operator()(const std::vector<std::size_t>& I, const std::vector<std::size_t>& J, DenseM_t& B) const {
    if (B.rows() != I.size() || B.cols() != J.size()) throw std::invalid_argument("Kernel::operator(): B has the wrong size");
    for (std::size_t j = 0; j < J.size(); j++)
      for (std::size_t i = 0; i < I.size(); i++) B(i, j) = eval(I[i], J[j]);
  }

  // kernel ridge regression: weights = (K + lambda I)^{-1} labels through an HSS approximation of K
  // (labels are permuted to the cluster order in place, as in the reference)
  DenseM_t fit_HSS(std::vector<scalar_t>& labels, const HSS::HSSOptions<scalar_t>& opts);
  // prediction[c] = sum_r weights(r) k(x_r, test_c)
  std::vector<scalar_t> predict(const DenseM_t& test, const DenseM_t& weights) const;

  // ---- extension: the fitted model kept for what a Gaussian-process reading of the fit needs (Kernel.cpp).
  // keep_model(true) before fit_HSS: the fit then keeps the factored HSS matrix, the cluster-ordered points in HBM, the permuted
  // labels and the weights until the next fit, keep_model(false) or the destructor.  Off by default: the fit and its memory
  // are then what they were.  Built-in kernels only (device_type() >= 0); every call below throws without a kept model.
  void keep_model(bool keep);
  bool has_model() const;
  // log|det(H)|, H the compressed K + lambda I, from the ULV factors (HSSMatrix::logabsdet)
  scalar_t logabsdet() const;
  // -1/2 y^T alpha - 1/2 log|det H| - n/2 log(2 pi), y the permuted labels, alpha the weights (the dot product in long double)
  scalar_t log_marginal_likelihood() const;
  // var[c] = k(t_c, t_c) - k_c^T H^-1 k_c, k_c = k(X, t_c): the variance of the latent function at the test points (add lambda
  // for the observation noise).  Not clamped: H is K + lambda I only up to the compression tolerance, so a value may come out
  // slightly negative.  Chunks of 64 test points: cross-kernel block, device solve in place, column-weighted sum.
  std::vector<scalar_t> predict_variance(const DenseM_t& test) const;
  // ---- extension: gradients in the test points (hssk_kernel_predict_grad).  Gauss and Laplace, d <= 64; every call
  // throws for a user-defined kernel, an ANOVA kernel and d > 64.
  // grad(j, c) = sum_r weights(r) dk(x_r, t_c) / dt_cj, d x m: the gradient of predict in the test points (no kept model needed)
  DenseM_t predict_gradient(const DenseM_t& test, const DenseM_t& weights) const;
  // predict_variance with grad(:, c) = -2 sum_r V(r, c) dk(x_r, t_c) / dt_c, V = H^-1 k(X, T) the solved columns of the chunk (the
  // term dk(t, t) / dt is 0 for these stationary kernels); grad is resized to d x m.  This is the derivative of the returned variance
  // exactly when H is symmetric; otherwise it is -2 D^T H^-1 k, D the derivative of k(X, t) in t.  The variances returned are bit
  // for bit those of predict_variance.
  std::vector<scalar_t> predict_variance_gradient(const DenseM_t& test, DenseM_t& grad) const;
  // a new lambda without a new compression: shift(lambda - current), factor, solve of the kept labels; returns the new weights,
  // which the model keeps, and lambda() is the new one afterwards
  DenseM_t model_set_lambda(scalar_t lambda);
  // the kept matrix through HSSMatrix::write (with the current lambda on the diagonal of its leaves)
  void model_write(const std::string& path) const;
  const std::vector<scalar_t>& model_labels() const;
  const DenseM_t& model_weights() const;
  // device-clock milliseconds of the last predict_variance: cross-kernel blocks, solves, column sums (profiling)
  const double* variance_ms() const { return var_ms_; }
  // The gradient of the log marginal likelihood in h and lambda (Gauss and Laplace):
  //   dL/dh = 1/2 alpha^T K' alpha - 1/2 tr(H^-1 K'),   dL/dlambda = 1/2 alpha^T alpha - 1/2 tr(H^-1),
  // K' = dK/dh the EXACT kernel derivative (hssk_kernel_matmul, never stored), H^-1 the kept, compressed and factored matrix:
  // the gradient of the exact-kernel likelihood evaluated with the compressed inverse, biased at a loose compression tolerance.
  // The traces are estimated with the columns z_k of Z (n x m, m >= 1, rows in the model's cluster order) as the mean of
  // s_k^T K' z_k and s_k^T z_k, s_k = H^-1 z_k: exact for the n probes sqrt(n) e_k, unbiased for Rademacher probes.  Columns go
  // in blocks of 64 with alpha as one column of the first, so 63 probes cost one pass over the pairs.
  LmlGradient log_marginal_likelihood_gradient(const DenseM_t& Z) const;
  // the same with the Rademacher block model_probes(m, seed)
  LmlGradient log_marginal_likelihood_gradient(int m = 63, unsigned long long seed = 0) const;
  // The gradient in one length scale per coordinate (automatic relevance determination; Gauss and Laplace, d <= 64).
  // k_l(x, y) = k(x / l, y / l), theta_j = ln l_j at l = 1, i.e. on the points the model holds:
  //   dL/dtheta_j = 1/2 alpha^T K_j alpha - 1/2 tr(H^-1 K_j),   K_j = K o D_j,  sum_j K_j = h dK/dh,
  // K_j the EXACT matrices (hssk_kernel_matmul_coord: one pass over the pairs per group of coordinates), H^-1 the kept, compressed
  // inverse as above, with the same bias at a loose tolerance.  Probes, blocks and alpha's place as in
  // log_marginal_likelihood_gradient; one ULV solve per block serves all coordinates.  A caller who fitted on X / w has
  // dL/dw_j = dtheta[j] / w_j.  gradient_ms() reports this call too.
  LmlGradientCoords log_marginal_likelihood_gradient_coords(const DenseM_t& Z) const;
  LmlGradientCoords log_marginal_likelihood_gradient_coords(int m = 63, unsigned long long seed = 0) const;
  // n x m entries +-1 from std::mt19937_64(seed), one bit per entry, column by column
  DenseM_t model_probes(int m, unsigned long long seed) const;
  // ||y - (K + lambda I) alpha||_2 / ||y||_2 with the EXACT kernel matrix (one product; the norms in long double)
  scalar_t model_residual() const;
  // device-clock milliseconds of the last gradient call: kernel products, solves, column dot products (profiling)
  const double* gradient_ms() const { return grad_ms_; }
  // ---- extension: solves with the EXACT K + lambda I, the kept ULV factors as preconditioner (Gauss and Laplace).
  // Right-preconditioned restarted GMRES, device resident, up to 64 columns in lockstep: per step one ULV solve, one exact product
  // (hssk_kernel_matmul) and one orthogonalisation (hssk_krylov_orth), the small least-squares problems per column on the host.
  // A column is converged when its TRUE residual, computed at the start of a cycle, is at most rtol ||b||; the total number of
  // steps never exceeds maxit (not converging is reported, not thrown); restart + 6 blocks of n x 64 doubles come from the
  // device pool for the length of the call.  Throws for rtol <= 0 or not finite, maxit < 1, restart < 1, an ANOVA kernel.
  //
  // model_refine: the kept labels as right-hand side, the current weights as first iterate; the model's weights become the last
  // iterate (GMRES residuals do not increase), so model_weights(), model_residual() and the y^T alpha of
  // log_marginal_likelihood() follow.  logabsdet() -- and with it the second term of the likelihood -- stays that of the
  // COMPRESSED matrix.  model_set_lambda and a new fit replace the weights by the compressed solve again.
  KrylovInfo model_refine(scalar_t rtol = 1e-8, int maxit = 100, int restart = 30);
  // X = (K + lambda I)^-1 B for any number of columns (rows in cluster order), in blocks of 64, from the first iterate H^-1 b; the
  // model is not changed.  info (may be null): the per-column data concatenated, the counts summed.
  DenseM_t model_solve(const DenseM_t& B, KrylovInfo* info = nullptr, scalar_t rtol = 1e-8, int maxit = 100, int restart = 30) const;
  // predict_variance with the exact solve in place of the compressed one: var[c] = k(t_c, t_c) - k_c^T (K + lambda I)^-1 k_c up
  // to rtol.  Not clamped.
  std::vector<scalar_t> predict_variance_exact(const DenseM_t& test, KrylovInfo* info = nullptr, scalar_t rtol = 1e-8, int maxit = 100,
                                               int restart = 30) const;
  // predict_variance_gradient with the exact solve: V = (K + lambda I)^-1 k(X, T) up to rtol (K is symmetric: the derivative of the
  // returned variance up to rtol).  The variances are bit for bit those of predict_variance_exact; krylov_inner is respected as
  // there, the gradient sum itself is always FP64.
  std::vector<scalar_t> predict_variance_gradient_exact(const DenseM_t& test, DenseM_t& grad, KrylovInfo* info = nullptr, scalar_t rtol = 1e-8,
                                                        int maxit = 100, int restart = 30) const;
  // device-clock milliseconds of the last of these three calls: exact products, ULV solves, Krylov kernels (profiling)
  const double* krylov_ms() const { return kry_ms_; }
  // ---- extension: the JOINT predictive covariance of the test points from the kept model (Gauss and Laplace).
  //   C = k(T, T) - (Q + Q^T) / 2,   Q = k(T, X) V,   V = H^-1 k(X, T),   m x m for test = d x m, any d.
  // Per chunk of 64 test points on the model's stream, no host wait in between: the cross block on a grid over both point sets
  // (hssk_kernel_cross_split), the ULV solve in place, and the product of the rectangular cross block of ALL test points with
  // the solved columns on the FP64 matrix cores (hssk_kernel_cross_matmul) into the chunk's columns of Q.  The kept compressed
  // matrix is not exactly symmetric, so Q is symmetrised, once, at the end: C(a, b) == C(b, a) bit for bit.  The sums run in
  // another order than those of predict_variance: the diagonal agrees with it within the two calls' rounding bounds, NOT bit
  // for bit.  Not clamped (a loosely compressed fit can give an indefinite C).  n x 64 + 2 m^2 doubles come from the device
  // pool beside the test points; a pool that refuses them raises the pool's own error.  Throws without a kept model, for an
  // ANOVA kernel and for test points of the wrong dimension.
  DenseM_t predict_covariance(const DenseM_t& test) const;
  // the same with the exact solve in place of the compressed one (as predict_variance_exact: GMRES from H^-1 k on, krylov_inner
  // respected, not converging reported in info, not thrown)
  DenseM_t predict_covariance_exact(const DenseM_t& test, KrylovInfo* info = nullptr, scalar_t rtol = 1e-8, int maxit = 100,
                                    int restart = 30) const;
  // device-clock milliseconds of the last covariance call: cross-kernel blocks, ULV solves, products (profiling)
  const double* covariance_ms() const { return cov_ms_; }
  // ---- extension: mixed precision for these three calls.  Handle state, set like keep_model; FP64 is the default
  // and leaves every call what it was, bit for bit.  With FP32 the product inside a cycle is hssk_kernel_matmul_f32 (FP32 per
  // pair on the matrix cores, from float points prepared once per call); the product at a cycle's start -- the true residual,
  // the only place where convergence is declared -- stays FP64.  A column leaves its cycle when the Arnoldi estimate is at most
  // max(rtol ||b||, inner_rtol ||r||), r its true residual at the cycle's start: below the rounded operator's floor the estimate
  // means nothing.  If a column's true residual does not decrease from one cycle start to the next, the rest of that block's
  // call runs with the FP64 product (KrylovInfo::fallbacks; reported, not thrown).  inner_rtol must lie in (0, 1).  The calls
  // then also throw for d > 64.
  void krylov_inner(KrylovInner p, scalar_t inner_rtol = KRYLOV_INNER_RTOL_DEFAULT);
  KrylovInner krylov_inner() const { return inner_; }
  scalar_t krylov_inner_rtol() const { return inner_rtol_; }
  // of the last of the three calls: FP64 products, FP32 products, fallbacks, cycles, ms of FP64 products, ms of FP32 products
  const double* krylov_stats() const { return kry_stats_; }

  const DenseM_t& data() const { return data_; }
  DenseM_t& data() { return data_; }
  std::vector<int>& permutation() { return perm_; }
  const std::vector<int>& permutation() const { return perm_; }
  // the clustering already reordered data() in place (binary_tree_clustering); nothing left to move
  virtual void permute() {}

  scalar_t lambda() const { return lambda_; }
  // extension (tests): neighbour lists (k x n, 0-based ids in cluster order) that replace the device search of the
  // first compression round
  void set_neighbors(const int* ann, int k) { user_ann_.assign(ann, ann + (size_t)k * n()); user_k_ = k; }
  const int* neighbors() const { return user_ann_.empty() ? nullptr : user_ann_.data(); }
  int neighbor_count() const { return user_k_; }
  // device evaluation parameters: 0 Gauss, 1 Laplace, 2 ANOVA, -1 = user-defined (host only)
  virtual int device_type() const { return -1; }
  virtual scalar_t width() const { return 1.; }
  virtual int degree() const { return 1; }

 protected:
  DenseM_t& data_;
  scalar_t lambda_;
  std::vector<int> perm_, user_ann_;
  int user_k_ = 0;
  virtual scalar_t eval_kernel_function(const scalar_t* x, const scalar_t* y) const = 0;

 private:
  struct Model;   // HSS matrix, device points, labels, weights (KernelModel.hpp)
  std::unique_ptr<Model> model_;
  bool keep_model_ = false;
  mutable double var_ms_[3] = {0., 0., 0.};
  mutable double grad_ms_[3] = {0., 0., 0.};
  mutable double cov_ms_[3] = {0., 0., 0.};
  mutable double kry_ms_[4] = {0., 0., 0., 0.};
  mutable double kry_stats_[6] = {0., 0., 0., 0., 0., 0.};
  KrylovInner inner_ = KrylovInner::FP64;
  scalar_t inner_rtol_ = KRYLOV_INNER_RTOL_DEFAULT;
  const Model& model(const char* what) const;
  // the prologue of both gradients (KernelGradient.cpp): the model after the checks of the probes Z (and of d() <= dmax where dmax
  // is given); the block model_probes(m, seed) after the checks of the seeded form
  const Model& check_probes(const char* what, const DenseM_t& Z, std::size_t dmax = 0) const;
  DenseM_t seeded_probes(const char* what, int m, unsigned long long seed) const;
  struct KrylovWork;   // the device blocks of a Krylov call (KernelModel.hpp)
  const Model& krylov_model(const char* what, scalar_t rtol, int maxit, int restart) const;
  // one block of at most 64 columns: dX (first iterate in, last iterate out) and dB are n x nc device blocks, leading dimension n
  void krylov_block(const Model& M, KrylovWork& ws, int nc, double* dX, const double* dB, scalar_t rtol, int maxit, int restart,
                    KrylovInfo& info) const;
  void krylov_finish(const Model& M, KrylovInfo& info) const;
  // bytes of the prepared float points a call's work buffers carry (0 in FP64 mode), and their preparation
  std::size_t krylov_prep_bytes() const;
  void krylov_prepare(const Model& M, KrylovWork& ws) const;
  // the chunk loop of the variance calls; ws == nullptr: the compressed solve; grad != nullptr: also the gradient in the test
  // points (resized to d x m), from the chunk's solved columns
  std::vector<scalar_t> variance_chunks(const Model& M, const DenseM_t& test, KrylovWork* ws, scalar_t rtol, int maxit, int restart,
                                        KrylovInfo* info, DenseM_t* grad = nullptr) const;
  // the chunk loop of the covariance calls; ws == nullptr: the compressed solve
  DenseM_t covariance_chunks(const Model& M, const DenseM_t& test, KrylovWork* ws, scalar_t rtol, int maxit, int restart, KrylovInfo* info) const;
  // what the gradients in the test points take: throws for a user-defined or ANOVA kernel and for d > 64
  void require_point_gradient(const char* what) const;
};

template <typename scalar_t> class GaussKernel;
template <> class GaussKernel<double> : public Kernel<double> {
 public:
  GaussKernel(DenseMatrix<double>& data, double h, double lambda) : Kernel<double>(data, lambda), h_(h) {}
  int device_type() const override { return 0; }
  double width() const override { return h_; }

 protected:
  double h_;
  double eval_kernel_function(const double* x, const double* y) const override {
    double s = 0.;
    for (std::size_t i = 0; i < d(); i++) { double t = x[i] - y[i]; s += t * t; }
    return std::exp(-s / (2. * h_ * h_));
  }
};

template <typename scalar_t> class LaplaceKernel;
template <> class LaplaceKernel<double> : public Kernel<double> {
 public:
  LaplaceKernel(DenseMatrix<double>& data, double h, double lambda) : Kernel<double>(data, lambda), h_(h) {}
  int device_type() const override { return 1; }
  double width() const override { return h_; }

 protected:
  double h_;
  double eval_kernel_function(const double* x, const double* y) const override {
    double s = 0.;
    for (std::size_t i = 0; i < d(); i++) s += std::abs(x[i] - y[i]);
    return std::exp(-s / h_);
  }
};

template <typename scalar_t> class ANOVAKernel;
template <> class ANOVAKernel<double> : public Kernel<double> {
 public:
  ANOVAKernel(DenseMatrix<double>& data, double h, double lambda, int p = 1) : Kernel<double>(data, lambda), h_(h), p_(p) {
    if (p < 1 || p > int(d())) throw std::invalid_argument("ANOVAKernel: degree must be in [1, d]");
  }
  int device_type() const override { return 2; }
  double width() const override { return h_; }
  int degree() const override { return p_; }

 protected:
  double h_;
  int p_;
  double eval_kernel_function(const double* x, const double* y) const override {
    std::vector<double> Kss(p_, 0.), Kpp(p_ + 1);
    for (std::size_t i = 0; i < d(); i++) {
      const double t = x[i] - y[i], tmp = std::exp(-(t * t) / (2. * h_ * h_));
      double pw = tmp;
      for (int j = 0; j < p_; j++) { Kss[j] += pw; pw *= tmp; }
    }
    Kpp[0] = 1.;
    for (int i = 1; i <= p_; i++) {
      double s = 0.;
      for (int q = 1; q <= i; q++) s += ((q & 1) ? 1. : -1.) * Kpp[i - q] * Kss[q - 1];
      Kpp[i] = s / i;
    }
    return Kpp[p_];
  }
};

// ---- single precision -------------------------------------------------------------------------------------------------
// Same members as the double class.  The FIT is promoted: points and labels are widened exactly, the FP64 front end runs
// unchanged (clustering, neighbours, compression, ULV, solve) and the solution is rounded once to float.  PREDICTION is
// native FP32 on the device (hssk_kernel_predict_f32).  After a fit the cluster-ordered points and the weights stay in HBM
// (device pool) until the next fit or the destructor: a prediction then uploads test points only.
template <> class Kernel<float> {
  using scalar_t = float;
  using DenseM_t = DenseMatrix<float>;

 public:
  Kernel(DenseM_t& data, scalar_t lambda);
  virtual ~Kernel();
  Kernel(const Kernel&) = delete;
  Kernel& operator=(const Kernel&) = delete;

  std::size_t n() const { return data_.cols(); }
  std::size_t d() const { return data_.rows(); }

  virtual scalar_t eval(std::size_t i, std::size_t j) const {
    return eval_kernel_function(data_.ptr(0, i), data_.ptr(0, j)) + ((i == j) ? lambda_ : scalar_t(0.));
  }
  void operator()(const std::vector<std::size_t>& I, const std::vector<std::size_t>& J, DenseM_t& B) const {
    if (B.rows() != I.size() || B.cols() != J.size()) throw std::invalid_argument("Kernel::operator(): B has the wrong size");
    for (std::size_t j = 0; j < J.size(); j++)
      for (std::size_t i = 0; i < I.size(); i++) B(i, j) = eval(I[i], J[j]);
  }

  // labels and data() are permuted to the cluster order in place, as in the double class
  DenseM_t fit_HSS(std::vector<scalar_t>& labels, const HSS::HSSOptions<scalar_t>& opts);
  // extension: the promoted fit with its own (double) options, so that tolerances need not pass through a float
  DenseM_t fit_HSS(std::vector<scalar_t>& labels, const HSS::HSSOptions<double>& opts);
  // prediction[c] = sum_r weights(r) k(x_r, test_c); the weights are uploaded, the points only if data() is not the resident copy
  std::vector<scalar_t> predict(const DenseM_t& test, const DenseM_t& weights) const;
  // extensions: the same with the weights of the last fit, which are resident (test points are the only upload);
  // predict_device: test (d x m) and prediction (m) already in HBM, no host copy of either; non-zero without a fit
  std::vector<scalar_t> predict(const DenseM_t& test) const;
  int predict_device(int m, const scalar_t* dtest, scalar_t* dpred) const;
  bool fitted() const;
  // of the last prediction: [0] tiles on the matrix cores, [1] tiles in the difference form, [2] splits of the training set,
  // [3] device-clock microseconds of the launches, [4] bytes uploaded, [5] 1 if the model was already resident
  const long long* predict_stats() const { return pstats_; }

  const DenseM_t& data() const { return data_; }
  DenseM_t& data() { return data_; }
  std::vector<int>& permutation() { return perm_; }
  const std::vector<int>& permutation() const { return perm_; }
  virtual void permute() {}

  scalar_t lambda() const { return lambda_; }
  void set_neighbors(const int* ann, int k) { user_ann_.assign(ann, ann + (size_t)k * n()); user_k_ = k; }
  const int* neighbors() const { return user_ann_.empty() ? nullptr : user_ann_.data(); }
  int neighbor_count() const { return user_k_; }
  virtual int device_type() const { return -1; }
  virtual scalar_t width() const { return 1.f; }
  virtual int degree() const { return 1; }
  // the kernel function itself (what a user-defined subclass supplies)
  scalar_t kernel_function(const scalar_t* x, const scalar_t* y) const { return eval_kernel_function(x, y); }

 protected:
  DenseM_t& data_;
  scalar_t lambda_;
  std::vector<int> perm_, user_ann_;
  int user_k_ = 0;
  virtual scalar_t eval_kernel_function(const scalar_t* x, const scalar_t* y) const = 0;

 private:
  struct Resident;   // device context, points and weights in HBM (KernelFloat.cpp)
  mutable std::unique_ptr<Resident> res_;
  mutable long long pstats_[6] = {0, 0, 0, 0, 0, 0};
  void run_predict(int m, const scalar_t* test_host, int ldt, const scalar_t* test_dev, const scalar_t* weights_host,
                   scalar_t* out_host, scalar_t* out_dev) const;
};

template <> class GaussKernel<float> : public Kernel<float> {
 public:
  GaussKernel(DenseMatrix<float>& data, float h, float lambda) : Kernel<float>(data, lambda), h_(h) {}
  int device_type() const override { return 0; }
  float width() const override { return h_; }

 protected:
  float h_;
  float eval_kernel_function(const float* x, const float* y) const override {
    float s = 0.f;
    for (std::size_t i = 0; i < d(); i++) { float t = x[i] - y[i]; s += t * t; }
    return std::exp(-s / (2.f * h_ * h_));
  }
};

template <> class LaplaceKernel<float> : public Kernel<float> {
 public:
  LaplaceKernel(DenseMatrix<float>& data, float h, float lambda) : Kernel<float>(data, lambda), h_(h) {}
  int device_type() const override { return 1; }
  float width() const override { return h_; }

 protected:
  float h_;
  float eval_kernel_function(const float* x, const float* y) const override {
    float s = 0.f;
    for (std::size_t i = 0; i < d(); i++) s += std::abs(x[i] - y[i]);
    return std::exp(-s / h_);
  }
};

template <> class ANOVAKernel<float> : public Kernel<float> {
 public:
  ANOVAKernel(DenseMatrix<float>& data, float h, float lambda, int p = 1) : Kernel<float>(data, lambda), h_(h), p_(p) {
    if (p < 1 || p > int(d())) throw std::invalid_argument("ANOVAKernel: degree must be in [1, d]");
  }
  int device_type() const override { return 2; }
  float width() const override { return h_; }
  int degree() const override { return p_; }

 protected:
  float h_;
  int p_;
  float eval_kernel_function(const float* x, const float* y) const override {
    std::vector<float> Kss(p_, 0.f), Kpp(p_ + 1);
    for (std::size_t i = 0; i < d(); i++) {
      const float t = x[i] - y[i], tmp = std::exp(-(t * t) / (2.f * h_ * h_));
      float pw = tmp;
      for (int j = 0; j < p_; j++) { Kss[j] += pw; pw *= tmp; }
    }
    Kpp[0] = 1.f;
    for (int i = 1; i <= p_; i++) {
      float s = 0.f;
      for (int q = 1; q <= i; q++) s += ((q & 1) ? 1.f : -1.f) * Kpp[i - q] * Kss[q - 1];
      Kpp[i] = s / i;
    }
    return Kpp[p_];
  }
};

template <typename scalar_t>
std::unique_ptr<Kernel<scalar_t>> create_kernel(KernelType k, DenseMatrix<scalar_t>& data, scalar_t h, scalar_t lambda, int p = 1) {
  switch (k) {
    case KernelType::LAPLACE: return std::unique_ptr<Kernel<scalar_t>>(new LaplaceKernel<scalar_t>(data, h, lambda));
    case KernelType::ANOVA: return std::unique_ptr<Kernel<scalar_t>>(new ANOVAKernel<scalar_t>(data, h, lambda, p));
    case KernelType::GAUSS:
    default: return std::unique_ptr<Kernel<scalar_t>>(new GaussKernel<scalar_t>(data, h, lambda));
  }
}

}  // namespace kernel
}  // namespace strumpack
