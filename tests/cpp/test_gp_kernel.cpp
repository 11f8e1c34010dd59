// kernel::Kernel<double> with a kept model, end to end through the C++ members: keep_model, fit_HSS, logabsdet,
// log_marginal_likelihood, predict_variance, model_set_lambda, model_write, and HSSMatrix<double>::logabsdet with its refusals
// (child view, shift).  The yardstick is dense algebra on the host (LU with partial pivoting) on the dense form of the
// COMPRESSED matrix -- HSSMatrix::read(model_write(...)).dense(), HSSMatrix::dense() -- so that what is compared is the
// factorization and the sweeps, not how well the compression met its tolerance, and the bounds are those of
// tests/gp_cases.py with the condition number estimated here.   usage: test_gp_kernel <n>
#include <cstdio>
#include <cmath>
#include <iostream>
#include <random>
#include <vector>

#include "HSS/HSSMatrix.hpp"
#include "kernel/Kernel.hpp"
#include "kernel/KernelRegression.hpp"

using namespace strumpack;

// rational quadratic kernel: only its virtual evaluation is known, so no model is kept for it
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

// dense yardstick: P A = L U in place, solves with A and A^T, log|det A|, and cond_2(A) as ||A||_F (an upper bound of the largest
// singular value) times 1 / sigma_min from 30 steps of inverse iteration on A^T A (converged to a few per cent: from below)
struct Dense {
  int n;
  std::vector<double> A, LU;
  std::vector<int> piv;
  double logdet = 0., normF = 0., inv2 = 0.;
  explicit Dense(const DenseMatrix<double>& M) : n((int)M.rows()), A((size_t)n * n), piv(n) {
    for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) { A[i + (size_t)j * n] = M(i, j); normF += M(i, j) * M(i, j); }
    normF = std::sqrt(normF);
    LU = A;
    for (int k = 0; k < n; k++) {
      int p = k;
      for (int i = k + 1; i < n; i++) if (std::abs(LU[i + (size_t)k * n]) > std::abs(LU[p + (size_t)k * n])) p = i;
      piv[k] = p;
      if (p != k) for (int j = 0; j < n; j++) std::swap(LU[k + (size_t)j * n], LU[p + (size_t)j * n]);
      const double d = LU[k + (size_t)k * n];
      logdet += std::log(std::abs(d));
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
  std::vector<double> mult(const std::vector<double>& x) const {
    std::vector<double> y(n, 0.);
    for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) y[i] += A[i + (size_t)j * n] * x[j];
    return y;
  }
};
static double norm2(const std::vector<double>& v) { double s = 0.; for (double x : v) s += x * x; return std::sqrt(s); }
template <class F> static bool throws(F&& f) {
  try { f(); } catch (const std::exception&) { return true; }
  return false;
}

int main(int argc, char* argv[]) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 300, d = 4, m = 70;
  std::mt19937 g(7);
  std::normal_distribution<double> u(0., 1.);
  DenseMatrix<double> X(d, n), T(d, m);
  for (int j = 0; j < n; j++) for (int i = 0; i < d; i++) X(i, j) = u(g);
  for (int j = 0; j < m; j++) for (int i = 0; i < d; i++) T(i, j) = u(g);
  std::vector<double> labels(n);
  for (int j = 0; j < n; j++) labels[j] = X(0, j) > 0. ? 1. : -1.;
  const double h = 1.1, lambda = 2., lambda2 = 0.5;
  HSS::HSSOptions<double> opts;
  opts.set_rel_tol(1e-9); opts.set_abs_tol(1e-12); opts.set_leaf_size(64);
  opts.set_clustering_algorithm(ClusteringAlgorithm::KD_TREE);
  opts.set_approximate_neighbors(64);
  const kernel::KernelType types[3] = {kernel::KernelType::GAUSS, kernel::KernelType::LAPLACE, kernel::KernelType::ANOVA};
  for (int t = 0; t < 3; t++) {
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(types[t], Xc, h, lambda, 2);
    if (K->has_model() || !throws([&] { K->logabsdet(); })) return fail("a model before keep_model");
    if (t == 0) {   // a plain fit keeps nothing
      DenseMatrix<double> Xp(X);
      std::vector<double> yp(labels);
      auto Kp = kernel::create_kernel<double>(types[t], Xp, h, lambda, 2);
      Kp->fit_HSS(yp, opts);
      if (Kp->has_model() || !throws([&] { Kp->predict_variance(T); })) return fail("a plain fit kept a model");
    }
    K->keep_model(true);
    auto w = K->fit_HSS(y, opts);
    if (!K->has_model()) return fail("keep_model(true) kept nothing");
    const std::string path = std::string(argc > 2 ? argv[2] : ".") + "/gp_kernel_model.bin";
    const double kmax = t == 2 ? d * (d - 1) / 2. : 1.;   // k(x, x): 1, or C(d, 2) for the ANOVA kernel of degree 2
    // full: log-determinant, likelihood and variance against an LU of the written matrix; otherwise the weights alone (O(n^2))
    auto check = [&](const DenseMatrix<double>& wk, const char* when, bool full) -> int {
      K->model_write(path);
      const DenseMatrix<double> Hd = HSS::HSSMatrix<double>::read(path).dense();
      std::remove(path.c_str());
      const std::string tag = "# " + kernel::get_name(types[t]) + " " + when + ": ";
      if (!full) {
        double nf = 0.;
        std::vector<double> r(n, 0.), wv(n);
        for (int j = 0; j < n; j++) { wv[j] = wk(j, 0); for (int i = 0; i < n; i++) { r[i] += Hd(i, j) * wk(j, 0); nf += Hd(i, j) * Hd(i, j); } }
        for (int i = 0; i < n; i++) r[i] -= y[i];
        const double be = norm2(r) / (std::sqrt(nf) * norm2(wv) + norm2(y));
        std::cout << tag << "backward error of the weights " << be << std::endl;
        return be <= 1e-13 ? 0 : fail("weights");
      }
      const Dense D(Hd);
      const double cond = D.cond(), tol_ld = 1e-12 * n * cond;   // |tr(H^-1 dH)| <= n cond ||dH|| / ||H||, tests/gp_cases.py
      const double got = K->logabsdet();
      std::cout << tag << "log det " << got << " dense " << D.logdet << " |error| " << std::abs(got - D.logdet) << " bound " << tol_ld
                << " (cond " << cond << ")" << std::endl;
      if (std::abs(got - D.logdet) > tol_ld) return fail("logabsdet");
      // the weights: backward error against the written matrix (the project's bound for the ULV solve)
      std::vector<double> wv(n);
      for (int i = 0; i < n; i++) wv[i] = wk(i, 0);
      std::vector<double> r = D.mult(wv);
      long double ya = 0.L;
      for (int i = 0; i < n; i++) { r[i] -= y[i]; ya += (long double)y[i] * (long double)wv[i]; }
      const double be = norm2(r) / (D.normF * norm2(wv) + norm2(y));
      std::cout << tag << "backward error of the weights " << be << std::endl;
      if (be > 1e-13) return fail("weights");
      const double lml = (double)(-0.5L * ya - 0.5L * (long double)D.logdet - 0.5L * n * std::log(2.L * std::acos(-1.L)));
      const double tol_l = 0.5 * tol_ld + 1e-12 * cond * std::abs((double)ya);
      if (std::abs(K->log_marginal_likelihood() - lml) > tol_l) return fail("log_marginal_likelihood");
      // the variance of six test points (each costs a pair of triangular solves on the host).  Bound of tests/gp_cases.py: the
      // forward error of the solve, 1e-12 cond ||kt|| ||z|| -- twice, the LU solve of the yardstick is no better --, and the
      // entry errors b = 256 * 2^-53 k(x, x) of the kernel values on both sides: 2 sum |z_r| b + ||Hd^-1|| ||kt|| sqrt(n) b
      auto var = K->predict_variance(T);
      double worst = 0.;
      for (int c = 0; c < 6 && c < m; c++) {
        std::vector<double> kt(n);
        DenseMatrix<double> pt(d, n + 1);
        for (int i = 0; i < n; i++) for (int k = 0; k < d; k++) pt(k, i) = Xc(k, i);
        for (int k = 0; k < d; k++) pt(k, n) = T(k, c);
        auto Kt = kernel::create_kernel<double>(types[t], pt, h, 0., 2);
        for (int i = 0; i < n; i++) kt[i] = Kt->eval(i, n);
        std::vector<double> z(kt);
        D.solve(z, false);
        double q = 0., z1 = 0.;
        for (int i = 0; i < n; i++) { q += kt[i] * z[i]; z1 += std::abs(z[i]); }
        const double b = 256. * 1.1102230246251565e-16 * kmax;
        const double bound = 2e-12 * cond * norm2(kt) * norm2(z) + 2. * z1 * b + D.inv2 * norm2(kt) * std::sqrt((double)n) * b;
        const double err = std::abs(var[c] - (Kt->eval(n, n) - q));
        worst = std::max(worst, err / bound);
        if (err > bound) { std::cout << tag << "variance error " << err << " bound " << bound << std::endl; return fail("predict_variance"); }
      }
      std::cout << tag << "largest variance error / bound " << worst << std::endl;
      return 0;
    };
    if (check(w, "fit", true)) return 1;
    auto p1 = K->predict(T, w);
    auto w2 = K->model_set_lambda(lambda2);
    if (K->lambda() != lambda2) return fail("model_set_lambda did not move lambda");
    if (check(w2, "set_lambda", t == 0)) return 1;
    for (int i = 0; i < n; i++) if (K->model_weights()(i, 0) != w2(i, 0)) return fail("the model keeps other weights than it returned");
    auto p2 = K->predict(T, K->model_weights());
    bool moved = false;
    for (int c = 0; c < m; c++) moved = moved || p1[c] != p2[c];
    if (!moved) return fail("predictions did not follow the new weights");
    K->keep_model(false);
    if (K->has_model() || !throws([&] { K->log_marginal_likelihood(); })) return fail("keep_model(false) kept the model");
  }
  {   // a user-defined kernel: the fit works, no model
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    CauchyKernel K(Xc, h, lambda);
    K.keep_model(true);
    K.fit_HSS(y, opts);
    if (K.has_model() || !throws([&] { K.logabsdet(); })) return fail("a user-defined kernel kept a model");
  }
  {   // the structured matrix itself: a child view and a shifted matrix refuse
    const int nt = 256;
    DenseMatrix<double> A(nt, nt);
    for (int j = 0; j < nt; j++) for (int i = 0; i < nt; i++) A(i, j) = 3.7 / (1. + std::abs(i - j));
    HSS::HSSOptions<double> o;
    o.set_rel_tol(1e-10); o.set_abs_tol(1e-13); o.set_leaf_size(32);
    HSS::HSSMatrix<double> H(A, o);
    if (!throws([&] { H.logabsdet(); })) return fail("logabsdet before factor");
    H.factor();
    const Dense D(H.dense());
    const double got = H.logabsdet(), tol = 1e-12 * nt * D.cond();
    std::cout << "# Toeplitz: log det " << got << " dense " << D.logdet << " bound " << tol << std::endl;
    if (std::abs(got - D.logdet) > tol) return fail("HSSMatrix::logabsdet");
    if (!throws([&] { H.child(0)->logabsdet(); })) return fail("logabsdet on a child view");
    H.child(0)->factor();
    if (!throws([&] { H.child(0)->logabsdet(); }) || !throws([&] { H.logabsdet(); })) return fail("logabsdet after a child's factorization");
    H.factor();
    H.shift(1.);
    if (!throws([&] { H.logabsdet(); })) return fail("logabsdet after shift");
  }
  std::cout << "# exiting" << std::endl;
  return 0;
}
