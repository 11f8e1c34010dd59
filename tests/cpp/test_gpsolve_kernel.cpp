// kernel::Kernel<double>: model_refine, model_solve and predict_variance_exact of a kept model through the C++ members, against
// dense algebra on the host.  The yardstick is an LU of the EXACT kernel matrix K + lambda I, entry by entry from the kernel's own
// formula; the bounds are those of tests/gpsolve_cases.py with the condition number estimated here and a flat entry bound for the
// kernel values (an entry within 512 * 2^-53 of its value, n roundings in a row of the product).  The fit runs at a loose
// compression tolerance, so that the compressed weights are visibly not the exact ones.   usage: test_gpsolve_kernel <n> [dir]
#include <cmath>
#include <cstdio>
#include <iostream>
#include <random>
#include <vector>

#include "HSS/HSSMatrix.hpp"
#include "kernel/Kernel.hpp"

using namespace strumpack;

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
template <class F> static bool throws(F&& f) {
  try { f(); } catch (const std::exception&) { return true; }
  return false;
}
static double norm2(const std::vector<double>& v) { double s = 0.; for (double x : v) s += x * x; return std::sqrt(s); }

// P A = L U, solves with A (symmetric here), cond_2 estimated as ||A||_F / sigma_min (30 steps of inverse iteration)
struct Dense {
  int n;
  std::vector<double> A, LU;
  std::vector<int> piv;
  double normF = 0., inv2 = 0.;
  explicit Dense(const std::vector<double>& M, int n_) : n(n_), A(M), LU(M), piv(n_) {
    for (double v : M) normF += v * v;
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
      const double s = norm2(x);
      for (double& v : x) v /= s;
      solve(x);
      inv2 = norm2(x);
    }
  }
  double cond() const { return normF * inv2; }
  void solve(std::vector<double>& b) const {
    for (int k = 0; k < n; k++) std::swap(b[k], b[piv[k]]);
    for (int j = 0; j < n; j++) for (int i = j + 1; i < n; i++) b[i] -= LU[i + (size_t)j * n] * b[j];
    for (int j = n - 1; j >= 0; j--) { b[j] /= LU[j + (size_t)j * n]; for (int i = 0; i < j; i++) b[i] -= LU[i + (size_t)j * n] * b[j]; }
  }
  // ||b - A x|| / ||b|| in long double, and ||x||_1
  double residual(const double* x, const double* b, double* x1) const {
    long double num = 0.L, den = 0.L, s1 = 0.L;
    for (int i = 0; i < n; i++) {
      long double r = b[i];
      for (int j = 0; j < n; j++) r -= (long double)A[i + (size_t)j * n] * x[j];
      num += r * r;
      den += (long double)b[i] * b[i];
      s1 += std::abs(x[i]);
    }
    *x1 = (double)s1;
    return den > 0 ? (double)std::sqrt(num / den) : 0.;
  }
};

int main(int argc, char* argv[]) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 300, d = 4, m = 70, mt = 70;
  const double U53 = 1.1102230246251565e-16, rtol = 1e-10;
  std::mt19937 g(11);
  std::normal_distribution<double> u(0., 1.);
  DenseMatrix<double> X(d, n);
  for (int j = 0; j < n; j++) for (int i = 0; i < d; i++) X(i, j) = u(g);
  std::vector<double> labels(n);
  for (int j = 0; j < n; j++) labels[j] = X(0, j) > 0. ? 1. : -1.;
  DenseMatrix<double> T(d, mt);
  for (int j = 0; j < mt; j++) for (int i = 0; i < d; i++) T(i, j) = u(g);
  const double h = 1.1, lambda = 0.5;
  HSS::HSSOptions<double> opts;
  opts.set_rel_tol(1e-2); opts.set_abs_tol(1e-10); opts.set_leaf_size(64);
  opts.set_clustering_algorithm(ClusteringAlgorithm::KD_TREE);
  opts.set_approximate_neighbors(64);
  const kernel::KernelType types[2] = {kernel::KernelType::GAUSS, kernel::KernelType::LAPLACE};
  for (int t = 0; t < 2; t++) {
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(types[t], Xc, h, lambda, 1);
    if (!throws([&] { K->model_refine(); }) || !throws([&] { K->model_solve(DenseMatrix<double>(n, 1)); }) ||
        !throws([&] { K->predict_variance_exact(T); }))
      return fail("a solve without a kept model");
    K->keep_model(true);
    K->fit_HSS(y, opts);
    const std::string tag = "# " + kernel::get_name(types[t]) + ": ";
    auto kfun = [&](const double* a, const double* b) {
      double s = 0.;
      for (int k = 0; k < d; k++) { const double df = a[k] - b[k]; s += t == 0 ? df * df : std::abs(df); }
      return std::exp(-s * (t == 0 ? 1. / (2. * h * h) : 1. / h));
    };
    std::vector<double> Ke((size_t)n * n);
    for (int j = 0; j < n; j++)
      for (int i = 0; i < n; i++) Ke[i + (size_t)j * n] = kfun(Xc.ptr(0, i), Xc.ptr(0, j)) + (i == j ? lambda : 0.);
    const Dense D(Ke, n);
    const double cond = D.cond(), ld = K->logabsdet(), yn = norm2(y);
    // a row of the product: entries within 512 u of theirs, n roundings of the sum, against ||x||_1
    auto rbound = [&](double x1, double bnorm) { return (512. + n) * U53 * x1 * std::sqrt((double)n) / bnorm; };
    // ---- refusals leave the model alone
    const DenseMatrix<double> w0 = K->model_weights();
    if (!throws([&] { K->model_refine(0.); }) || !throws([&] { K->model_refine(-1.); }) || !throws([&] { K->model_refine(std::nan("")); }) ||
        !throws([&] { K->model_refine(1e-8, 0); }) || !throws([&] { K->model_refine(1e-8, 10, 0); }) ||
        !throws([&] { K->model_solve(DenseMatrix<double>(n - 1, 2)); }) || !throws([&] { K->predict_variance_exact(T, nullptr, 0.); }) ||
        !throws([&] { K->predict_variance_exact(DenseMatrix<double>(d + 1, 2)); }))
      return fail("a bad argument accepted");
    for (int i = 0; i < n; i++) if (K->model_weights()(i, 0) != w0(i, 0)) return fail("a refused call changed the weights");
    // ---- refine
    double x1 = 0.;
    const double before = D.residual(w0.data(), y.data(), &x1), got0 = K->model_residual();
    if (!(before >= 1e3 * rtol) || std::abs(got0 - before) > rbound(x1, yn)) return fail("the residual of the compressed weights");
    const kernel::KrylovInfo I = K->model_refine(rtol, 100, 30);
    const DenseMatrix<double>& w = K->model_weights();
    const double after = D.residual(w.data(), y.data(), &x1), br = rbound(x1, yn);
    std::cout << tag << "refine: " << I.iterations << " steps, " << I.products << " products, " << I.solves << " solves, residual " << I.residual0[0]
              << " -> " << I.residual[0] << " (dense " << before << " -> " << after << ", bound " << br << ")" << std::endl;
    if (!I.converged || I.its.size() != 1 || I.its[0] != I.iterations || I.iterations < 1 || I.iterations > 100) return fail("refine: info");
    if (I.products != I.iterations + I.cycles + 1) return fail("refine: products");
    if (std::abs(I.residual[0] - after) > br || after > rtol + br || std::abs(I.residual0[0] - before) > rbound(x1, yn) + 1e-12 * before) return fail("refine: residual");
    if (std::abs(K->model_residual() - after) > br) return fail("model_residual after refine");
    {
      std::vector<double> xe(y);
      D.solve(xe);
      double e = 0.;
      for (int i = 0; i < n; i++) e += (w(i, 0) - xe[i]) * (w(i, 0) - xe[i]);
      const double fe = std::sqrt(e) / norm2(xe), fb = cond * (rtol + br + 2e-12);
      std::cout << tag << "refine: forward error " << fe << " bound " << fb << " (cond " << cond << ")" << std::endl;
      if (fe > fb) return fail("refine: forward error");
    }
    if (K->logabsdet() != ld) return fail("refine changed the log-determinant");
    const kernel::KrylovInfo I2 = K->model_refine(rtol, 100, 30);
    if (!I2.converged || I2.iterations != 0 || I2.products != 1 || I2.cycles != 0) return fail("a second refine");
    if (!(K->krylov_ms()[0] > 0.)) return fail("krylov_ms");
    // ---- solve: 70 columns (64 + 6), the labels first, an exactly zero column
    DenseMatrix<double> B(n, m);
    for (int c = 0; c < m; c++) for (int i = 0; i < n; i++) B(i, c) = c == 0 ? y[i] : (c == 5 ? 0. : u(g));
    kernel::KrylovInfo IS;
    const DenseMatrix<double> S = K->model_solve(B, &IS, rtol, 100, 30);
    if (!IS.converged || (int)IS.its.size() != m || (int)IS.residual.size() != m) return fail("solve: info");
    double worst = 0.;
    int most = 0;
    for (int c = 0; c < m; c++) {
      if (c == 5) {
        for (int i = 0; i < n; i++) if (S(i, c) != 0.) return fail("solve: the zero column");
        if (IS.its[c] != 0 || IS.residual[c] != 0.) return fail("solve: the zero column's info");
        continue;
      }
      std::vector<double> b(B.ptr(0, c), B.ptr(0, c) + n), xe(b);
      const double r = D.residual(S.ptr(0, c), b.data(), &x1), bb = rbound(x1, norm2(b));
      if (std::abs(IS.residual[c] - r) > bb || r > rtol + bb) return fail("solve: residual");
      D.solve(xe);
      double e = 0.;
      for (int i = 0; i < n; i++) { if (!std::isfinite(S(i, c))) return fail("solve: not a number"); e += (S(i, c) - xe[i]) * (S(i, c) - xe[i]); }
      const double fe = std::sqrt(e) / norm2(xe);
      worst = std::max(worst, fe / (cond * (rtol + bb + 2e-12)));
      most = std::max(most, IS.its[c]);
    }
    std::cout << tag << "solve: " << most << " steps at most, largest forward error / bound " << worst << std::endl;
    if (worst > 1. || most != IS.iterations) return fail("solve: forward error");
    for (int i = 0; i < n; i++) if (K->model_weights()(i, 0) != w(i, 0)) return fail("solve changed the weights");
    // ---- exact variance against k_tt - k^T (K + lambda I)^-1 k
    kernel::KrylovInfo IV;
    const std::vector<double> ve = K->predict_variance_exact(T, &IV, rtol, 100, 30), vc = K->predict_variance(T);
    if ((int)ve.size() != mt || !IV.converged || (int)IV.its.size() != mt) return fail("variance: info");
    double gap = 0., wv = 0., bmax = 0.;
    for (int c = 0; c < mt; c++) {
      std::vector<double> k(n), z;
      for (int i = 0; i < n; i++) k[i] = kfun(Xc.ptr(0, i), T.ptr(0, c));
      z = k;
      D.solve(z);
      long double q = 0.L, z1 = 0.L;
      for (int i = 0; i < n; i++) { q += (long double)k[i] * z[i]; z1 += std::abs(z[i]); }
      const double ref = 1. - (double)q, nk = norm2(k), nz = norm2(z);
      // the solve's residual through the inverse, both dense solves, the entries of k (twice) and the n-term sum
      const double bv = rtol * nk * nk * D.inv2 + 2e-12 * cond * nk * nz + 2. * 512. * U53 * (double)z1 + D.inv2 * nk * 512. * U53 * std::sqrt((double)n) +
                        n * U53 * nk * nz;
      wv = std::max(wv, std::abs(ve[c] - ref) / bv);
      bmax = std::max(bmax, bv);
      if (ve[c] < -bv) return fail("variance: negative beyond the bound");
      gap = std::max(gap, std::abs(ve[c] - vc[c]));
    }
    std::cout << tag << "exact variance: largest error / bound " << wv << ", largest bound " << bmax << ", largest gap to the compressed variance " << gap
              << std::endl;
    if (wv > 1.) return fail("variance: error");
    if (!(gap >= 1e3 * bmax)) return fail("the variance case proves nothing");   // (it could pass by returning the compressed values)
    const std::vector<double> vc2 = K->predict_variance(T);
    if (vc2 != vc) return fail("the compressed variance changed");
    // ---- after a new lambda the weights are the compressed ones again
    K->model_set_lambda(0.7);
    if (!(K->model_residual() >= 1e3 * rtol)) return fail("set_lambda kept the refined weights");
    K->keep_model(false);
    if (!throws([&] { K->model_refine(); })) return fail("keep_model(false) kept the model");
  }
  {   // ANOVA: a model, but no product
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(kernel::KernelType::ANOVA, Xc, h, lambda, 2);
    K->keep_model(true);
    K->fit_HSS(y, opts);
    const double ld = K->logabsdet();
    if (!throws([&] { K->model_refine(); }) || !throws([&] { K->model_solve(DenseMatrix<double>(n, 1)); }) || !throws([&] { K->predict_variance_exact(T); }))
      return fail("an ANOVA solve");
    if (K->logabsdet() != ld) return fail("a refused call disturbed the ANOVA model");
  }
  {   // a user-defined kernel keeps no model
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    CauchyKernel K(Xc, h, lambda);
    K.keep_model(true);
    K.fit_HSS(y, opts);
    if (!throws([&] { K.model_refine(); }) || !throws([&] { K.model_solve(DenseMatrix<double>(n, 1)); })) return fail("a user-defined kernel answered");
  }
  std::cout << "# exiting" << std::endl;
  return 0;
}
