// kernel::Kernel<double>: the gradients of the predicted mean and variance in the test points, end to end through the C++ members
// predict_gradient, predict_variance_gradient and predict_variance_gradient_exact.  The yardstick is dense algebra on
// the host: the derivative of every pair in long double, an LU with partial pivoting of the dense form of the COMPRESSED matrix
// (HSSMatrix::read(model_write(...)).dense()) for the compressed variance, and of the exact K + lambda I for the exact one.  The
// bounds are those of tests/predgrad_cases.py with the condition number estimated here and a flat 256 * 2^-53 for the entry error of
// a kernel value, as in test_gp_kernel.cpp.   usage: test_predgrad_kernel <n> [directory for the model file]
#include <cstdio>
#include <cmath>
#include <iostream>
#include <random>
#include <vector>

#include "HSS/HSSMatrix.hpp"
#include "kernel/Kernel.hpp"
#include "kernel/KernelRegression.hpp"

using namespace strumpack;

// rational quadratic kernel: only its virtual evaluation is known, so there is no gradient for it
class CauchyKernel : public kernel::Kernel<double> {
 public:
  CauchyKernel(DenseMatrix<double>& data, double h, double lambda) : Kernel<double>(data, lambda), h_(h) {}

 protected:
  double h_;
  double eval_kernel_function(const double* x, const double* y) const override {
    double s = 0.;
    for (std::size_t k = 0; k < this->d(); k++) s += (x[k] - y[k]) * (x[k] - y[k]);
    return 1. / (1. + s / (h_ * h_));
  }
};

static int fail(const char* what) { std::cout << "ERROR: " << what << std::endl; return 1; }

// dense yardstick: P A = L U in place, solves with A, and cond_2(A) as ||A||_F (an upper bound of the largest singular value) times
// 1 / sigma_min from 30 steps of inverse iteration on A^T A (converged to a few per cent: from below)
struct Dense {
  int n;
  std::vector<double> LU;
  std::vector<int> piv;
  double normF = 0., inv2 = 0.;
  template <class M> explicit Dense(int n_, const M& entry) : n(n_), LU((size_t)n_ * n_), piv(n_) {
    for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) { const double v = entry(i, j); LU[i + (size_t)j * n] = v; normF += v * v; }
    normF = std::sqrt(normF);
    for (int k = 0; k < n; k++) {
      int p = k;
      for (int i = k + 1; i < n; i++) if (std::abs(LU[i + (size_t)k * n]) > std::abs(LU[p + (size_t)k * n])) p = i;
      piv[k] = p;
      if (p != k) for (int j = 0; j < n; j++) std::swap(LU[k + (size_t)j * n], LU[p + (size_t)j * n]);
      const double d = LU[k + (size_t)k * n];
      for (int i = k + 1; i < n; i++) LU[i + (size_t)k * n] /= d;
      for (int j = k + 1; j < n; j++) {
        const double u = LU[k + (size_t)j * n];
        double* c = &LU[(size_t)j * n];
        const double* l = &LU[(size_t)k * n];
        for (int i = k + 1; i < n; i++) c[i] -= l[i] * u;
      }
    }
    std::vector<double> x(n, 1.);
    for (int it = 0; it < 30; it++) {
      double s = 0.;
      for (double v : x) s += v * v;
      s = std::sqrt(s);
      for (double& v : x) v /= s;
      solve(x, true);
      solve(x, false);   // x <- (A^T A)^-1 x
      s = 0.;
      for (double v : x) s += v * v;
      inv2 = std::sqrt(std::sqrt(s));   // ||(A^T A)^-1 x|| -> 1 / sigma_min^2
    }
  }
  double cond() const { return normF * inv2; }
  void solve(std::vector<double>& b, bool trans) const {
    if (!trans) {
      for (int k = 0; k < n; k++) std::swap(b[k], b[piv[k]]);
      for (int j = 0; j < n; j++) for (int i = j + 1; i < n; i++) b[i] -= LU[i + (size_t)j * n] * b[j];
      for (int j = n - 1; j >= 0; j--) { b[j] /= LU[j + (size_t)j * n]; for (int i = 0; i < j; i++) b[i] -= LU[i + (size_t)j * n] * b[j]; }
    } else {
      for (int j = 0; j < n; j++) { for (int i = 0; i < j; i++) b[j] -= LU[i + (size_t)j * n] * b[i]; b[j] /= LU[j + (size_t)j * n]; }
      for (int j = n - 1; j >= 0; j--) for (int i = j + 1; i < n; i++) b[j] -= LU[i + (size_t)j * n] * b[i];
      for (int k = n - 1; k >= 0; k--) std::swap(b[k], b[piv[k]]);
    }
  }
};
static double norm2(const std::vector<double>& v) { double s = 0.; for (double x : v) s += x * x; return std::sqrt(s); }
template <class F> static bool throws(F&& f) {
  try { f(); } catch (const std::exception&) { return true; }
  return false;
}

static const double U = 1.1102230246251565e-16;   // 2^-53

// the derivative of the pair (x, t) in t, coordinate by coordinate, in long double: D[j]; and the bound of one term without its
// weight, bD[j] = u (16 + (d + 4) a) |D[j]| (the exponent a moved by (d + 4) u relative, 16 u for the exponential, the factor and
// the term: what tests/predgrad_cases.py derives, rounded up)
static void pair_deriv(bool laplace, int d, double h, const double* x, const double* t, std::vector<long double>& D, std::vector<double>& bD,
                       double& k) {
  long double a = 0.L;
  for (int j = 0; j < d; j++) { const long double df = (long double)x[j] - (long double)t[j]; a += laplace ? std::fabs(df) : df * df; }
  a = laplace ? a / h : a / (2.L * h * h);
  const long double kk = std::exp(-a), f = laplace ? kk / h : kk / ((long double)h * h);
  k = (double)kk;
  for (int j = 0; j < d; j++) {
    const long double df = (long double)x[j] - (long double)t[j];
    D[j] = laplace ? f * (df > 0 ? 1.L : (df < 0 ? -1.L : 0.L)) : f * df;
    bD[j] = U * (16. + (d + 4) * (double)a) * (double)std::fabs(D[j]);
  }
}

int main(int argc, char* argv[]) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 300, d = 4, m = 70, mv = 6;
  std::mt19937 g(11);
  std::normal_distribution<double> u(0., 1.);
  DenseMatrix<double> X(d, n), T(d, m);
  for (int j = 0; j < n; j++) for (int i = 0; i < d; i++) X(i, j) = u(g);
  for (int j = 0; j < m; j++) for (int i = 0; i < d; i++) T(i, j) = u(g);
  for (int i = 0; i < d; i++) T(i, m - 1) = X(i, 3);   // the last test point is a training point
  std::vector<double> labels(n);
  for (int j = 0; j < n; j++) labels[j] = X(0, j) > 0. ? 1. : -1.;
  const double h = 1.1, lambda = 2.;
  const double nsum = n + (n + 63) / 64;   // roundings of a sum over the training points and over the most splits there can be
  HSS::HSSOptions<double> opts;
  opts.set_rel_tol(1e-9); opts.set_abs_tol(1e-12); opts.set_leaf_size(64);
  opts.set_clustering_algorithm(ClusteringAlgorithm::KD_TREE);
  opts.set_approximate_neighbors(64);
  const std::string path = std::string(argc > 2 ? argv[2] : ".") + "/predgrad_kernel_model.bin";
  const kernel::KernelType types[2] = {kernel::KernelType::GAUSS, kernel::KernelType::LAPLACE};
  for (int t = 0; t < 2; t++) {
    const bool laplace = t == 1;
    const std::string tag = "# " + kernel::get_name(types[t]) + ": ";
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(types[t], Xc, h, lambda);
    DenseMatrix<double> gv;
    if (!throws([&] { K->predict_variance_gradient(T, gv); })) return fail("a variance gradient without a kept model");
    K->keep_model(true);
    auto w = K->fit_HSS(y, opts);
    // ---- the mean: every entry against the long double sum
    const DenseMatrix<double> G = K->predict_gradient(T, w);
    if ((int)G.rows() != d || (int)G.cols() != m) return fail("predict_gradient: shape");
    std::vector<long double> D(d);
    std::vector<double> bD(d);
    double worst = 0., kv = 0.;
    for (int c = 0; c < m; c++) {
      std::vector<long double> ref(d, 0.L);
      std::vector<double> bound(d, 0.), mag(d, 0.);
      for (int r = 0; r < n; r++) {
        pair_deriv(laplace, d, h, Xc.ptr(0, r), T.ptr(0, c), D, bD, kv);
        for (int j = 0; j < d; j++) { ref[j] += (long double)w(r, 0) * D[j]; bound[j] += std::abs(w(r, 0)) * bD[j]; mag[j] += std::abs(w(r, 0)) * (double)std::fabs(D[j]); }
      }
      for (int j = 0; j < d; j++) {
        const double b = bound[j] + nsum * U * mag[j], err = (double)std::fabs((long double)G(j, c) - ref[j]);
        worst = std::max(worst, err / b);
        if (err > b) { std::cout << tag << "mean gradient error " << err << " bound " << b << std::endl; return fail("predict_gradient"); }
      }
    }
    std::cout << tag << "largest mean gradient error / bound " << worst << std::endl;
    const DenseMatrix<double> G2 = K->predict_gradient(T, w);
    for (int c = 0; c < m; c++) for (int j = 0; j < d; j++) if (G(j, c) != G2(j, c)) return fail("two predict_gradient calls differ");
    // ---- the variance: -2 D^T A^-1 k for the first mv test points against an LU of A (each costs a pair of triangular solves)
    DenseMatrix<double> Tv(d, mv, T, 0, 0);
    auto check_variance = [&](const Dense& A, const DenseMatrix<double>& got, const std::vector<double>& res, const char* what) -> int {
      const double cond = A.cond(), b = 256. * U;
      double wv = 0.;
      for (int c = 0; c < mv; c++) {
        std::vector<double> kt(n), Dm((size_t)n * d), bDm((size_t)n * d);
        for (int r = 0; r < n; r++) {
          pair_deriv(laplace, d, h, Xc.ptr(0, r), Tv.ptr(0, c), D, bD, kt[r]);
          for (int j = 0; j < d; j++) { Dm[r + (size_t)j * n] = (double)D[j]; bDm[r + (size_t)j * n] = bD[j]; }
        }
        std::vector<double> z(kt);
        A.solve(z, false);
        for (int j = 0; j < d; j++) {
          long double ref = 0.L;
          double zb = 0., zd = 0., nD = 0.;
          for (int r = 0; r < n; r++) {
            const double Dr = Dm[r + (size_t)j * n];
            ref += (long double)z[r] * Dr;
            zb += std::abs(z[r]) * bDm[r + (size_t)j * n];
            zd += std::abs(z[r] * Dr);
            nD += Dr * Dr;
          }
          nD = std::sqrt(nD);
          // (the forward error twice: the LU solve of the yardstick is no better than the ULV solve)
          const double bound = 2. * (2e-12 * cond * nD * norm2(z) + zb + A.inv2 * nD * std::sqrt((double)n) * b + nsum * U * zd)
                               + res[c] * 2. * cond * nD * norm2(kt);
          const double err = std::abs(got(j, c) - (double)(-2.L * ref));
          wv = std::max(wv, err / bound);
          if (err > bound) { std::cout << tag << what << " error " << err << " bound " << bound << std::endl; return 1; }
        }
      }
      std::cout << tag << "largest " << what << " error / bound " << wv << " (cond " << cond << ")" << std::endl;
      return 0;
    };
    K->model_write(path);
    const DenseMatrix<double> Hd = HSS::HSSMatrix<double>::read(path).dense();
    std::remove(path.c_str());
    const std::vector<double> var = K->predict_variance_gradient(Tv, gv), var0 = K->predict_variance(Tv);
    if ((int)gv.rows() != d || (int)gv.cols() != mv) return fail("predict_variance_gradient: shape");
    for (int c = 0; c < mv; c++) if (var[c] != var0[c]) return fail("the variances next to the gradient are not those of predict_variance");
    {
      const Dense A(n, [&](int i, int j) { return Hd(i, j); });
      if (check_variance(A, gv, std::vector<double>(mv, 0.), "variance gradient")) return fail("predict_variance_gradient");
      // all 70 test points (chunks of 64 and 6): the same columns under the same bound (the solve of a chunk of 64 columns need
      // not agree bit for bit with that of 6)
      DenseMatrix<double> gall;
      const std::vector<double> vall = K->predict_variance_gradient(T, gall), vall0 = K->predict_variance(T);
      if ((int)gall.cols() != m) return fail("predict_variance_gradient: shape of the long call");
      for (int c = 0; c < m; c++) if (vall[c] != vall0[c]) return fail("the variances next to the gradient are not those of predict_variance (70 points)");
      if (check_variance(A, gall, std::vector<double>(mv, 0.), "variance gradient (70 points)")) return fail("predict_variance_gradient, 70 points");
    }
    if (t == 0) {   // the exact solve against the exact K + lambda I (eval carries lambda on the diagonal)
      kernel::KrylovInfo info;
      DenseMatrix<double> ge;
      const std::vector<double> ve = K->predict_variance_gradient_exact(Tv, ge, &info, 1e-10, 200, 30), ve0 = K->predict_variance_exact(Tv, nullptr, 1e-10, 200, 30);
      if (!info.converged) return fail("predict_variance_gradient_exact did not converge");
      for (int c = 0; c < mv; c++) if (ve[c] != ve0[c]) return fail("the variances next to the exact gradient are not those of predict_variance_exact");
      const Dense E(n, [&](int i, int j) { return K->eval(i, j); });
      if (check_variance(E, ge, info.residual, "exact variance gradient")) return fail("predict_variance_gradient_exact");
    }
    K->keep_model(false);
    if (!throws([&] { K->predict_variance_gradient(T, gv); })) return fail("keep_model(false) kept the model");
  }
  {   // the refusals: an ANOVA kernel, a user-defined kernel, wrong shapes
    DenseMatrix<double> Xc(X);
    auto A = kernel::create_kernel<double>(kernel::KernelType::ANOVA, Xc, h, lambda, 2);
    DenseMatrix<double> w(n, 1), wbad(n - 1, 1), Tbad(d + 1, 3), gv;
    if (!throws([&] { A->predict_gradient(T, w); })) return fail("an ANOVA kernel gave a gradient");
    CauchyKernel C(Xc, h, lambda);
    if (!throws([&] { C.predict_gradient(T, w); })) return fail("a user-defined kernel gave a gradient");
    auto Gk = kernel::create_kernel<double>(kernel::KernelType::GAUSS, Xc, h, lambda);
    if (!throws([&] { Gk->predict_gradient(Tbad, w); }) || !throws([&] { Gk->predict_gradient(T, wbad); })) return fail("predict_gradient took a wrong shape");
    const DenseMatrix<double> none = Gk->predict_gradient(DenseMatrix<double>(d, 0), w);
    if ((int)none.rows() != d || none.cols() != 0) return fail("no test points");
  }
  std::cout << "# exiting" << std::endl;
  return 0;
}
