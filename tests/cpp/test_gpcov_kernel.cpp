// kernel::Kernel<double>: the joint predictive covariance of a set of test points, end to end through the C++ members
// predict_covariance, predict_covariance_exact and covariance_ms.  The yardstick is dense algebra on the host: the
// kernel values in long double, an LU with partial pivoting of the dense form of the COMPRESSED matrix
// (HSSMatrix::read(model_write(...)).dense()) for the compressed covariance, and of the exact K + lambda I for the exact one:
//     C_ref(a, b) = k(t_a, t_b) - (Q(a, b) + Q(b, a)) / 2,   Q(a, b) = k_a^T A^-1 k_b.
// The bounds are those of tests/gpcov_cases.py with the condition number estimated here and a flat 256 * 2^-53 for the entry error
// of a kernel value, as in test_gp_kernel.cpp.   usage: test_gpcov_kernel <n> [directory for the model file]
#include <cstdio>
#include <cmath>
#include <iostream>
#include <random>
#include <vector>

#include "HSS/HSSMatrix.hpp"
#include "kernel/Kernel.hpp"
#include "kernel/KernelRegression.hpp"

using namespace strumpack;

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

static double pair_value(bool laplace, int d, double h, const double* x, const double* t) {
  long double a = 0.L;
  for (int j = 0; j < d; j++) { const long double df = (long double)x[j] - (long double)t[j]; a += laplace ? std::fabs(df) : df * df; }
  return (double)std::exp(-(laplace ? a / h : a / (2.L * h * h)));
}

int main(int argc, char* argv[]) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 300, d = 4, m = 70;
  std::mt19937 g(13);
  std::normal_distribution<double> u(0., 1.);
  DenseMatrix<double> X(d, n), T(d, m);
  for (int j = 0; j < n; j++) for (int i = 0; i < d; i++) X(i, j) = u(g);
  for (int j = 0; j < m; j++) for (int i = 0; i < d; i++) T(i, j) = u(g);
  for (int i = 0; i < d; i++) T(i, m - 1) = X(i, 3);   // the last test point is a training point
  std::vector<double> labels(n);
  for (int j = 0; j < n; j++) labels[j] = X(0, j) > 0. ? 1. : -1.;
  const double h = 1.1, lambda = 2.;
  const double nsum = n + (n + 15) / 16;   // roundings of a sum over the training points and over the most splits there can be
  HSS::HSSOptions<double> opts;
  opts.set_rel_tol(1e-9); opts.set_abs_tol(1e-12); opts.set_leaf_size(64);
  opts.set_clustering_algorithm(ClusteringAlgorithm::KD_TREE);
  opts.set_approximate_neighbors(64);
  const std::string path = std::string(argc > 2 ? argv[2] : ".") + "/gpcov_kernel_model.bin";
  const kernel::KernelType types[2] = {kernel::KernelType::GAUSS, kernel::KernelType::LAPLACE};
  for (int t = 0; t < 2; t++) {
    const bool laplace = t == 1;
    const std::string tag = "# " + kernel::get_name(types[t]) + ": ";
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(types[t], Xc, h, lambda);
    if (!throws([&] { K->predict_covariance(T); })) return fail("a covariance without a kept model");
    K->keep_model(true);
    K->fit_HSS(y, opts);
    // the cross-kernel columns and k(T, T) in long double
    std::vector<std::vector<double>> kt(m, std::vector<double>(n));
    for (int c = 0; c < m; c++) for (int r = 0; r < n; r++) kt[c][r] = pair_value(laplace, d, h, Xc.ptr(0, r), T.ptr(0, c));
    // got against k(T, T) - (Q + Q^T) / 2 with A^-1 from the LU; res: the final relative residual per column (exact solve)
    auto check = [&](const Dense& A, const DenseMatrix<double>& got, const std::vector<double>& res, const char* what) -> int {
      if ((int)got.rows() != m || (int)got.cols() != m) { std::cout << tag << what << ": shape" << std::endl; return 1; }
      for (int b = 0; b < m; b++) for (int a = 0; a < m; a++) if (got(a, b) != got(b, a)) { std::cout << tag << what << ": not symmetric" << std::endl; return 1; }
      const double cond = A.cond(), eb = 256. * U;
      std::vector<std::vector<double>> z(kt);
      std::vector<double> nk(m), nz(m);
      for (int c = 0; c < m; c++) { A.solve(z[c], false); nk[c] = norm2(kt[c]); nz[c] = norm2(z[c]); }
      std::vector<double> Q((size_t)m * m), B((size_t)m * m);
      for (int b = 0; b < m; b++)
        for (int a = 0; a < m; a++) {
          long double q = 0.L;
          double za = 0., zk = 0.;
          for (int r = 0; r < n; r++) { q += (long double)kt[a][r] * z[b][r]; za += std::abs(z[b][r]); zk += std::abs(kt[a][r] * z[b][r]); }
          Q[a + (size_t)b * m] = (double)q;
          // (the forward error twice: the LU solve of the yardstick is no better than the ULV solve)
          B[a + (size_t)b * m] = 2. * (2e-12 * cond * nk[a] * nz[b] + za * eb + A.inv2 * nk[a] * std::sqrt((double)n) * eb + nsum * U * zk)
                                 + res[b] * A.inv2 * nk[b] * nk[a];
        }
      double worst = 0.;
      for (int b = 0; b < m; b++)
        for (int a = 0; a < m; a++) {
          const double ref = pair_value(laplace, d, h, T.ptr(0, a), T.ptr(0, b)) - 0.5 * (Q[a + (size_t)b * m] + Q[b + (size_t)a * m]);
          const double bound = 0.5 * (B[a + (size_t)b * m] + B[b + (size_t)a * m]) + eb, err = std::abs(got(a, b) - ref);
          worst = std::max(worst, err / bound);
          if (err > bound) { std::cout << tag << what << " (" << a << ", " << b << ") error " << err << " bound " << bound << std::endl; return 1; }
        }
      std::cout << tag << "largest " << what << " error / bound " << worst << " (cond " << cond << ")" << std::endl;
      return 0;
    };
    K->model_write(path);
    const DenseMatrix<double> Hd = HSS::HSSMatrix<double>::read(path).dense();
    std::remove(path.c_str());
    const std::vector<double> var0 = K->predict_variance(T);
    const DenseMatrix<double> C = K->predict_covariance(T);
    const std::vector<double> var1 = K->predict_variance(T);
    for (int c = 0; c < m; c++) if (var0[c] != var1[c]) return fail("predict_covariance changed what predict_variance returns");
    {
      const Dense A(n, [&](int i, int j) { return Hd(i, j); });
      if (check(A, C, std::vector<double>(m, 0.), "covariance")) return fail("predict_covariance");
    }
    const DenseMatrix<double> C2 = K->predict_covariance(T);
    for (int b = 0; b < m; b++) for (int a = 0; a < m; a++) if (C(a, b) != C2(a, b)) return fail("two predict_covariance calls differ");
    const double* ms = K->covariance_ms();
    std::cout << tag << "covariance_ms " << ms[0] << " " << ms[1] << " " << ms[2] << std::endl;
    if (!(ms[0] >= 0. && ms[1] >= 0. && ms[2] >= 0.) || !(ms[0] + ms[1] + ms[2] > 0.)) return fail("covariance_ms");
    if (t == 0) {   // the exact solve against the exact K + lambda I (eval carries lambda on the diagonal)
      kernel::KrylovInfo info;
      const DenseMatrix<double> Ce = K->predict_covariance_exact(T, &info, 1e-10, 200, 30);
      if (!info.converged || (int)info.residual.size() != m) return fail("predict_covariance_exact did not converge");
      if (info.solves < 2) return fail("predict_covariance_exact: one first solve per chunk expected");
      const Dense E(n, [&](int i, int j) { return K->eval(i, j); });
      if (check(E, Ce, info.residual, "exact covariance")) return fail("predict_covariance_exact");
    }
    const DenseMatrix<double> none = K->predict_covariance(DenseMatrix<double>(d, 0));
    if (none.rows() != 0 || none.cols() != 0) return fail("no test points");
    if (!throws([&] { K->predict_covariance(DenseMatrix<double>(d + 1, 3)); })) return fail("predict_covariance took a wrong dimension");
    if (!throws([&] { K->predict_covariance_exact(DenseMatrix<double>(d + 1, 3)); })) return fail("predict_covariance_exact took a wrong dimension");
    K->keep_model(false);
    if (!throws([&] { K->predict_covariance(T); })) return fail("keep_model(false) kept the model");
  }
  {   // an ANOVA fit keeps a model, but there is no exact product for it
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto A = kernel::create_kernel<double>(kernel::KernelType::ANOVA, Xc, h, lambda, 2);
    A->keep_model(true);
    A->fit_HSS(y, opts);
    if (!throws([&] { A->predict_covariance(T); }) || !throws([&] { A->predict_covariance_exact(T); })) return fail("an ANOVA kernel gave a covariance");
  }
  std::cout << "# exiting" << std::endl;
  return 0;
}
