// kernel::Kernel<double>::log_marginal_likelihood_gradient_coords: the gradient of the log marginal likelihood in one length scale
// per coordinate through the C++ members, against dense algebra on the host, and the C entry point SPX_kernel_lml_gradient_coords
// on a handle fitted with the same options, bit for bit.  Yardsticks as in test_gpgrad_kernel.cpp: an LU of the dense form of the
// COMPRESSED matrix for the solves, the kernel's formula entry by entry for K_j = K o D_j, the bounds of tests/gpard_cases.py with
// the condition number estimated here and a flat entry bound.  Probes beyond the first six are checked through the traces only.
//   usage: test_gpard_kernel <n> <scratch directory>
#include <cmath>
#include <cstdio>
#include <iostream>
#include <random>
#include <vector>

#include "HSS/HSSMatrix.hpp"
#include "kernel/Kernel.h"
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

// P A = L U, solves with A and A^T, cond_2 estimated as ||A||_F / sigma_min (30 steps of inverse iteration on A^T A)
struct Dense {
  int n;
  std::vector<double> LU;
  std::vector<int> piv;
  double normF = 0., inv2 = 0.;
  explicit Dense(const DenseMatrix<double>& M) : n((int)M.rows()), LU((size_t)n * n), piv(n) {
    for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) { LU[i + (size_t)j * n] = M(i, j); normF += M(i, j) * M(i, j); }
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
      solve(x, true);
      solve(x, false);
      inv2 = std::sqrt(norm2(x));
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

int main(int argc, char* argv[]) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 300, d = 4, m = 70, full = 6;
  std::mt19937 g(11);
  std::normal_distribution<double> u(0., 1.);
  DenseMatrix<double> X(d, n);
  for (int j = 0; j < n; j++) for (int i = 0; i < d; i++) X(i, j) = u(g);
  std::vector<double> labels(n);
  for (int j = 0; j < n; j++) labels[j] = X(0, j) + 0.5 * X(2, j) > 0. ? 1. : -1.;
  const double h = 1.1, lambda = 2.;
  // one set of options for the C++ class and the C handle: the C interface's defaults, then the same command line
  const char* args[] = {"kernel", "--hss_rel_tol", "1e-4", "--hss_abs_tol", "1e-10", "--hss_leaf_size", "64"};
  const int nargs = sizeof(args) / sizeof(args[0]);
  std::vector<char*> av;
  for (const char* a : args) av.push_back(const_cast<char*>(a));
  HSS::HSSOptions<double> opts;
  opts.set_verbose(false);
  opts.set_clustering_algorithm(ClusteringAlgorithm::COBBLE);
  opts.set_from_command_line(nargs, av.data());
  const kernel::KernelType types[2] = {kernel::KernelType::GAUSS, kernel::KernelType::LAPLACE};
  for (int t = 0; t < 2; t++) {
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(types[t], Xc, h, lambda, 1);
    if (!throws([&] { K->log_marginal_likelihood_gradient_coords(); })) return fail("a coordinate gradient without a kept model");
    K->keep_model(true);
    auto w = K->fit_HSS(y, opts);
    const std::string tag = "# " + kernel::get_name(types[t]) + ": ";
    const std::string path = std::string(argc > 2 ? argv[2] : ".") + "/gpard_kernel_model.bin";
    K->model_write(path);
    const DenseMatrix<double> Hd = HSS::HSSMatrix<double>::read(path).dense();
    std::remove(path.c_str());
    const Dense D(Hd);
    const double cond = D.cond(), ld = K->logabsdet();
    // K_j entry by entry: k D_j
    std::vector<std::vector<double>> Kj(d, std::vector<double>((size_t)n * n));
    for (int j = 0; j < n; j++)
      for (int i = 0; i < n; i++) {
        double a = 0.;
        for (int k = 0; k < d; k++) { const double df = Xc(k, i) - Xc(k, j); a += t == 0 ? df * df : std::abs(df); }
        const double kv = std::exp(-a * (t == 0 ? 1. / (2. * h * h) : 1. / h));
        for (int k = 0; k < d; k++) {
          const double df = Xc(k, i) - Xc(k, j);
          Kj[k][i + (size_t)j * n] = kv * (t == 0 ? df * df / (h * h) : std::abs(df) / h);
        }
      }
    // an entry k D_j <= 2 a e^-a < 1 is within 64 * 2^-53 (1 + a) of its value relatively, at most 256 * 2^-53 absolutely, and the
    // n-term sums of the product add n 2^-53 per entry: one flat bound for both
    const double b = (256. + n) * 1.1102230246251565e-16;
    const DenseMatrix<double> Z = K->model_probes(m, 7);
    const kernel::LmlGradientCoords G = K->log_marginal_likelihood_gradient_coords(Z), G2 = K->log_marginal_likelihood_gradient_coords(m, 7);
    if (G.dtheta != G2.dtheta || G.quad != G2.quad || G.trace != G2.trace || G.tc != G2.tc) return fail("seeded and explicit gradients differ");
    if (G.m != m || (int)G.dtheta.size() != d || (int)G.quad.size() != d || (int)G.trace.size() != d || G.tc.size() != (size_t)d * m)
      return fail("sizes of the result");
    long double a1 = 0.L;
    for (int j = 0; j < n; j++) a1 += std::abs(w(j, 0));
    double worst = 0.;
    for (int c = 0; c < full; c++) {
      std::vector<double> s(n), z(n);
      for (int i = 0; i < n; i++) z[i] = s[i] = Z(i, c);
      D.solve(s, false);
      double s1 = 0.;
      for (int i = 0; i < n; i++) s1 += std::abs(s[i]);
      for (int k = 0; k < d; k++) {
        std::vector<double> gz(n, 0.);
        for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) gz[i] += Kj[k][i + (size_t)j * n] * z[j];
        double tc = 0.;
        for (int i = 0; i < n; i++) tc += s[i] * gz[i];
        const double bt = 2e-12 * cond * norm2(s) * norm2(gz) + s1 * b * n, got = G.tc[(size_t)k * m + c];
        worst = std::max(worst, std::abs(got - tc) / bt);
        if (std::abs(got - tc) > bt) {
          std::cout << tag << "coordinate " << k << " probe " << c << ": " << got << " dense " << tc << " bound " << bt << std::endl;
          return fail("per-probe values");
        }
      }
    }
    std::cout << tag << "largest per-probe error / bound " << worst << " (cond " << cond << ")" << std::endl;
    const kernel::LmlGradient Gh = K->log_marginal_likelihood_gradient(Z);
    double sq = 0., st = 0.;
    for (int k = 0; k < d; k++) {
      long double aka = 0.L;
      for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) aka += (long double)w(i, 0) * Kj[k][i + (size_t)j * n] * w(j, 0);
      const double bq = (double)(0.5L * a1 * a1) * b + 1e-13 * std::abs((double)aka);
      std::cout << tag << "coordinate " << k << ": quad " << G.quad[k] << " dense " << (double)(0.5L * aka) << " bound " << bq << ", trace "
                << G.trace[k] << ", dtheta " << G.dtheta[k] << std::endl;
      if (std::abs(G.quad[k] - (double)(0.5L * aka)) > bq) return fail("quad");
      double sum = 0.;
      for (int c = 0; c < m; c++) sum += G.tc[(size_t)k * m + c];
      if (std::abs(G.trace[k] - sum / m) > 1e-13 * std::abs(sum / m)) return fail("trace means");
      if (std::abs(G.dtheta[k] - (G.quad[k] - 0.5 * G.trace[k])) > 1e-15 * (std::abs(G.quad[k]) + std::abs(G.trace[k]))) return fail("assembly of the gradient");
      sq += G.quad[k];
      st += G.trace[k];
    }
    // the coordinates add up to h times the derivative in h: the same solves, products of the same entries in another order
    if (std::abs(sq - h * Gh.quad_h) > (double)(a1 * a1) * b * (d + 1) || std::abs(st - h * Gh.trace_h) > 1e-9 * std::abs(st))
      return fail("the sum over the coordinates is not h dL/dh");
    // the C entry point on a handle of its own, fitted with the same options: bit for bit
    {
      DenseMatrix<double> Xh(X);
      std::vector<double> yh(labels);
      STRUMPACKKernel C = STRUMPACK_create_kernel_double(n, d, Xh.data(), h, lambda, 1, t);
      if (!C || SPX_kernel_keep_model(C, 1)) return fail("the C handle");
      STRUMPACK_kernel_fit_HSS_double(C, yh.data(), nargs, av.data());
      std::vector<double> wc(n), grad(d, 0.), terms(2 * d + (size_t)d * m, 0.), grad2(d, 0.);
      if (SPX_kernel_weights(C, wc.data())) return fail("the C handle's weights");
      for (int i = 0; i < n; i++) if (wc[i] != w(i, 0)) return fail("the C handle's fit differs from the class's");
      if (SPX_kernel_lml_gradient_coords(C, m, Z.data(), 0, grad.data(), terms.data())) return fail("SPX_kernel_lml_gradient_coords");
      if (SPX_kernel_lml_gradient_coords(C, m, nullptr, 7, grad2.data(), nullptr)) return fail("SPX_kernel_lml_gradient_coords (seeded)");
      if (grad != G.dtheta || grad2 != G.dtheta) return fail("C and C++ gradients differ");
      for (int k = 0; k < d; k++) if (terms[k] != G.quad[k] || terms[d + k] != G.trace[k]) return fail("C and C++ terms differ");
      for (size_t e = 0; e < G.tc.size(); e++) if (terms[2 * d + e] != G.tc[e]) return fail("C and C++ per-probe values differ");
      std::vector<double> keep(grad);
      if (!SPX_kernel_lml_gradient_coords(C, 0, nullptr, 7, grad.data(), nullptr) || grad != keep) return fail("m = 0 through C");
      STRUMPACK_destroy_kernel_double(C);
    }
    // refusals leave the model alone
    if (!throws([&] { K->log_marginal_likelihood_gradient_coords(0, 1); })) return fail("m = 0 accepted");
    if (!throws([&] { K->log_marginal_likelihood_gradient_coords(DenseMatrix<double>(n - 1, 3)); })) return fail("a probe block of the wrong height accepted");
    if (!throws([&] { K->log_marginal_likelihood_gradient_coords(DenseMatrix<double>(n, 0)); })) return fail("an empty probe block accepted");
    if (K->logabsdet() != ld) return fail("the gradient disturbed the kept model");
    const kernel::LmlGradientCoords G3 = K->log_marginal_likelihood_gradient_coords(Z);
    if (G3.dtheta != G.dtheta || G3.tc != G.tc) return fail("two gradient calls differ");
    if (!(K->gradient_ms()[0] >= 0.)) return fail("gradient_ms");
    K->model_set_lambda(0.5);
    const kernel::LmlGradientCoords G4 = K->log_marginal_likelihood_gradient_coords(Z);
    if (G4.dtheta == G.dtheta) return fail("the gradient did not follow set_lambda");
    K->keep_model(false);
    if (!throws([&] { K->log_marginal_likelihood_gradient_coords(Z); })) return fail("keep_model(false) kept the model");
  }
  {   // ANOVA: a model, but no derivative
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(kernel::KernelType::ANOVA, Xc, h, lambda, 2);
    K->keep_model(true);
    K->fit_HSS(y, opts);
    const double ld = K->logabsdet();
    if (!throws([&] { K->log_marginal_likelihood_gradient_coords(5, 1); })) return fail("an ANOVA coordinate gradient");
    if (K->logabsdet() != ld) return fail("a refused call disturbed the ANOVA model");
  }
  {   // 65 coordinates: the gradient in h answers, the coordinate gradient refuses
    const int d65 = 65;
    DenseMatrix<double> X65(d65, n);
    for (int j = 0; j < n; j++) for (int i = 0; i < d65; i++) X65(i, j) = u(g);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(kernel::KernelType::GAUSS, X65, 8., lambda, 1);
    K->keep_model(true);
    K->fit_HSS(y, opts);
    const double ld = K->logabsdet();
    if (!throws([&] { K->log_marginal_likelihood_gradient_coords(5, 1); })) return fail("a coordinate gradient in R^65");
    if (K->logabsdet() != ld || !std::isfinite(K->log_marginal_likelihood_gradient(5, 1).dh)) return fail("a refused call disturbed the R^65 model");
  }
  {   // a user-defined kernel keeps no model
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    CauchyKernel K(Xc, h, lambda);
    K.keep_model(true);
    K.fit_HSS(y, opts);
    if (!throws([&] { K.log_marginal_likelihood_gradient_coords(5, 1); })) return fail("a user-defined kernel answered");
  }
  std::cout << "# exiting" << std::endl;
  return 0;
}
