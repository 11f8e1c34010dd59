// kernel::Kernel<double> in mixed precision (krylov_inner(KrylovInner::FP32)): model_refine, model_solve and
// predict_variance_exact through the C++ members, against dense algebra on the host, as tests/cpp/test_gpsolve_kernel.cpp checks
// the FP64 mode -- the same yardstick (an LU of the exact K + lambda I), the same bounds, rtol unchanged: convergence is declared
// on the FP64 residual alone.  On top: the counts of the mixed mode (FP32 products = steps, FP64 products = cycles + 1 per block,
// no fallback), the setter and its refusals, and FP64 set explicitly against a handle that never set it, bit for bit.
// usage: test_gpmixed_kernel <n> [dir]
#include <cmath>
#include <cstdio>
#include <iostream>
#include <random>
#include <vector>

#include "HSS/HSSMatrix.hpp"
#include "kernel/Kernel.hpp"

using namespace strumpack;

static int fail(const char* what) { std::cout << "ERROR: " << what << std::endl; return 1; }
template <class F> static bool throws(F&& f) {
  try { f(); } catch (const std::exception&) { return true; }
  return false;
}
static double norm2(const std::vector<double>& v) { double s = 0.; for (double x : v) s += x * x; return std::sqrt(s); }

// P A = L U, solves with A, cond_2 estimated as ||A||_F / sigma_min (30 steps of inverse iteration)
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
        for (int i = k + 1; i < n; i++) LU[i + (size_t)j * n] -= LU[i + (size_t)k * n] * u;
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
  double residual(const double* x, const double* b, double* x1) const {   // ||b - A x|| / ||b|| in long double, and ||x||_1
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
  const int n = argc > 1 ? std::atoi(argv[1]) : 300, d = 4, m = 70, mt = 6;
  const double U53 = 1.1102230246251565e-16, rtol = 1e-8;
  std::mt19937 g(11);
  std::normal_distribution<double> u(0., 1.);
  DenseMatrix<double> X(d, n);
  // (a quarter of a standard normal cloud: within the width of the kernel, so that the Gauss product runs on the matrix cores)
  for (int j = 0; j < n; j++) for (int i = 0; i < d; i++) X(i, j) = 0.25 * u(g);
  std::vector<double> labels(n);
  for (int j = 0; j < n; j++) labels[j] = X(0, j) > 0. ? 1. : -1.;
  DenseMatrix<double> T(d, mt);
  for (int j = 0; j < mt; j++) for (int i = 0; i < d; i++) T(i, j) = 0.25 * u(g);
  const double h = 1.1, lambda = 0.5;
  HSS::HSSOptions<double> opts;
  opts.set_rel_tol(1e-2); opts.set_abs_tol(1e-10); opts.set_leaf_size(64);
  opts.set_clustering_algorithm(ClusteringAlgorithm::KD_TREE);
  opts.set_approximate_neighbors(64);
  const kernel::KernelType types[2] = {kernel::KernelType::GAUSS, kernel::KernelType::LAPLACE};
  for (int t = 0; t < 2; t++) {
    DenseMatrix<double> Xc(X), Xd(X);
    std::vector<double> y(labels), yd(labels);
    auto K = kernel::create_kernel<double>(types[t], Xc, h, lambda, 1);
    auto Kd = kernel::create_kernel<double>(types[t], Xd, h, lambda, 1);   // never sets a mode
    const std::string tag = "# " + kernel::get_name(types[t]) + ": ";
    // ---- the setter: state of the handle, before the fit as well
    if (K->krylov_inner() != kernel::KrylovInner::FP64 || K->krylov_inner_rtol() != kernel::KRYLOV_INNER_RTOL_DEFAULT) return fail("the default mode");
    K->krylov_inner(kernel::KrylovInner::FP32, 1e-3);
    if (!throws([&] { K->krylov_inner(kernel::KrylovInner::FP32, 0.); }) || !throws([&] { K->krylov_inner(kernel::KrylovInner::FP32, 1.); }) ||
        !throws([&] { K->krylov_inner(kernel::KrylovInner::FP64, -1e-4); }) || !throws([&] { K->krylov_inner(kernel::KrylovInner::FP32, std::nan("")); }) ||
        !throws([&] { K->krylov_inner(static_cast<kernel::KrylovInner>(7)); }))
      return fail("a bad mode accepted");
    if (K->krylov_inner() != kernel::KrylovInner::FP32 || K->krylov_inner_rtol() != 1e-3) return fail("a refused setter changed the mode");
    if (!throws([&] { K->model_refine(); })) return fail("a mixed solve without a kept model");
    K->keep_model(true);
    Kd->keep_model(true);
    K->fit_HSS(y, opts);
    Kd->fit_HSS(yd, opts);
    // ---- FP64 set explicitly is bitwise the handle that never set it
    K->krylov_inner(kernel::KrylovInner::FP64);
    {
      const kernel::KrylovInfo a = K->model_refine(rtol, 100, 30), b = Kd->model_refine(rtol, 100, 30);
      for (int i = 0; i < n; i++) if (K->model_weights()(i, 0) != Kd->model_weights()(i, 0)) return fail("FP64 set explicitly differs from the default");
      if (a.iterations != b.iterations || a.products != b.products || a.products32 != 0 || a.fallbacks != 0 || a.residual[0] != b.residual[0]) return fail("FP64 info");
      if (a.products != a.iterations + a.cycles + 1) return fail("FP64 products");
    }
    K->model_set_lambda(lambda);   // (the compressed weights are back)
    K->krylov_inner(kernel::KrylovInner::FP32);
    if (K->krylov_inner_rtol() != kernel::KRYLOV_INNER_RTOL_DEFAULT) return fail("the default inner_rtol");
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
    auto rbound = [&](double x1, double bnorm) { return (512. + n) * U53 * x1 * std::sqrt((double)n) / bnorm; };
    // ---- refine
    double x1 = 0.;
    const DenseMatrix<double> w0 = K->model_weights();
    const double before = D.residual(w0.data(), y.data(), &x1);
    if (!(before >= 1e3 * rtol)) return fail("the residual of the compressed weights");
    const kernel::KrylovInfo I = K->model_refine(rtol, 100, 30);
    const DenseMatrix<double>& w = K->model_weights();
    const double after = D.residual(w.data(), y.data(), &x1), br = rbound(x1, yn);
    std::cout << tag << "mixed refine: " << I.iterations << " steps, " << I.cycles << " cycles, " << I.products << " FP64 + " << I.products32
              << " FP32 products, residual " << I.residual0[0] << " -> " << I.residual[0] << " (dense " << before << " -> " << after << ")" << std::endl;
    if (!I.converged || I.its.size() != 1 || I.its[0] != I.iterations || I.iterations < 1) return fail("refine: info");
    if (I.fallbacks != 0 || I.products32 != I.iterations || I.products != I.cycles + 1) return fail("refine: counts");
    if (std::abs(I.residual[0] - after) > br || after > rtol + br) return fail("refine: residual");
    {
      std::vector<double> xe(y);
      D.solve(xe);
      double e = 0.;
      for (int i = 0; i < n; i++) e += (w(i, 0) - xe[i]) * (w(i, 0) - xe[i]);
      if (std::sqrt(e) / norm2(xe) > cond * (rtol + br + 2e-12)) return fail("refine: forward error");
    }
    if (K->logabsdet() != ld) return fail("refine changed the log-determinant");
    if (!(K->krylov_stats()[0] == (double)I.products && K->krylov_stats()[1] == (double)I.products32 && K->krylov_stats()[3] == (double)I.cycles)) return fail("krylov_stats");
    // ---- solve: 70 columns (64 + 6), an exactly zero column; two calls bit for bit
    DenseMatrix<double> B(n, m);
    for (int c = 0; c < m; c++) for (int i = 0; i < n; i++) B(i, c) = c == 0 ? y[i] : (c == 5 ? 0. : u(g));
    kernel::KrylovInfo IS, IS2;
    const DenseMatrix<double> S = K->model_solve(B, &IS, rtol, 100, 30), S2 = K->model_solve(B, &IS2, rtol, 100, 30);
    if (!IS.converged || (int)IS.its.size() != m || IS.fallbacks != 0 || IS.products != IS.cycles + 2 || IS.products32 < 1) return fail("solve: info");
    double worst = 0.;
    for (int c = 0; c < m; c++) {
      for (int i = 0; i < n; i++) if (S(i, c) != S2(i, c)) return fail("two mixed solves differ");
      if (c == 5) {
        for (int i = 0; i < n; i++) if (S(i, c) != 0.) return fail("solve: the zero column");
        continue;
      }
      std::vector<double> b(B.ptr(0, c), B.ptr(0, c) + n), xe(b);
      const double r = D.residual(S.ptr(0, c), b.data(), &x1), bb = rbound(x1, norm2(b));
      if (std::abs(IS.residual[c] - r) > bb || r > rtol + bb) return fail("solve: residual");
      D.solve(xe);
      double e = 0.;
      for (int i = 0; i < n; i++) e += (S(i, c) - xe[i]) * (S(i, c) - xe[i]);
      worst = std::max(worst, std::sqrt(e) / norm2(xe) / (cond * (rtol + bb + 2e-12)));
    }
    std::cout << tag << "mixed solve: " << IS.iterations << " steps at most, " << IS.products << " FP64 + " << IS.products32
              << " FP32 products, largest forward error / bound " << worst << std::endl;
    if (worst > 1.) return fail("solve: forward error");
    // ---- exact variance
    kernel::KrylovInfo IV;
    const std::vector<double> ve = K->predict_variance_exact(T, &IV, rtol, 100, 30);
    if ((int)ve.size() != mt || !IV.converged || IV.products32 < 1 || IV.fallbacks != 0) return fail("variance: info");
    for (int c = 0; c < mt; c++) {
      std::vector<double> k(n), z;
      for (int i = 0; i < n; i++) k[i] = kfun(Xc.ptr(0, i), T.ptr(0, c));
      z = k;
      D.solve(z);
      long double q = 0.L, z1 = 0.L;
      for (int i = 0; i < n; i++) { q += (long double)k[i] * z[i]; z1 += std::abs(z[i]); }
      const double ref = 1. - (double)q, nk = norm2(k), nz = norm2(z);
      const double bv = rtol * nk * nk * D.inv2 + 2e-12 * cond * nk * nz + 2. * 512. * U53 * (double)z1 + D.inv2 * nk * 512. * U53 * std::sqrt((double)n) +
                        n * U53 * nk * nz;
      if (std::abs(ve[c] - ref) > bv) return fail("variance: error");
    }
  }
  {   // ANOVA in mixed mode: the mode can be set, the calls are refused and leave the model alone
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(kernel::KernelType::ANOVA, Xc, h, lambda, 2);
    K->keep_model(true);
    K->krylov_inner(kernel::KrylovInner::FP32);
    K->fit_HSS(y, opts);
    const double ld = K->logabsdet();
    if (!throws([&] { K->model_refine(); }) || !throws([&] { K->model_solve(DenseMatrix<double>(n, 1)); }) || !throws([&] { K->predict_variance_exact(T); }))
      return fail("an ANOVA solve in mixed mode");
    if (K->logabsdet() != ld) return fail("a refused call disturbed the ANOVA model");
  }
  std::cout << "# exiting" << std::endl;
  return 0;
}
