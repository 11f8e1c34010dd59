// kernel::Kernel<double>: the gradient of the log marginal likelihood, the probes and the residual of a kept model through the
// C++ members, against dense algebra on the host.  The yardstick of the solve is an LU of the dense form of the COMPRESSED matrix
// (HSSMatrix::read(model_write(...)).dense()), the yardstick of the kernel derivative is Kernel::eval entry by entry; the bounds
// are those of tests/gpgrad_cases.py with the condition number estimated here and a flat entry bound for the kernel values.
// Probes beyond the first six are checked through the traces only (a host solve each).   usage: test_gpgrad_kernel <n>
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
  for (int j = 0; j < n; j++) labels[j] = X(0, j) > 0. ? 1. : -1.;
  const double h = 1.1, lambda = 2.;
  HSS::HSSOptions<double> opts;
  opts.set_rel_tol(1e-4); opts.set_abs_tol(1e-10); opts.set_leaf_size(64);
  opts.set_clustering_algorithm(ClusteringAlgorithm::KD_TREE);
  opts.set_approximate_neighbors(64);
  const kernel::KernelType types[2] = {kernel::KernelType::GAUSS, kernel::KernelType::LAPLACE};
  for (int t = 0; t < 2; t++) {
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(types[t], Xc, h, lambda, 1);
    if (!throws([&] { K->log_marginal_likelihood_gradient(); }) || !throws([&] { K->model_residual(); }) || !throws([&] { K->model_probes(3, 1); }))
      return fail("a gradient without a kept model");
    K->keep_model(true);
    auto w = K->fit_HSS(y, opts);
    const std::string tag = "# " + kernel::get_name(types[t]) + ": ";
    const std::string path = std::string(argc > 2 ? argv[2] : ".") + "/gpgrad_kernel_model.bin";
    K->model_write(path);
    const DenseMatrix<double> Hd = HSS::HSSMatrix<double>::read(path).dense();
    std::remove(path.c_str());
    const Dense D(Hd);
    const double cond = D.cond(), ld = K->logabsdet();
    // K' entry by entry from the kernel's own evaluation: k a c_h with a = -log k
    const double ch = t == 0 ? 2. / h : 1. / h;
    std::vector<double> Kp((size_t)n * n), Ke((size_t)n * n);
    for (int j = 0; j < n; j++)
      for (int i = 0; i < n; i++) {
        double a = 0.;
        for (int k = 0; k < d; k++) { const double df = Xc(k, i) - Xc(k, j); a += t == 0 ? df * df : std::abs(df); }
        a *= t == 0 ? 1. / (2. * h * h) : 1. / h;
        Ke[i + (size_t)j * n] = std::exp(-a);
        Kp[i + (size_t)j * n] = std::exp(-a) * a * ch;
      }
    // an entry of K' is within 64 * 2^-53 (1 + a) a c_h k <= 256 * 2^-53 c_h of its value (x^2 e^-x <= 0.55, x e^-x <= 0.37), and
    // the n-term sums of the product add n 2^-53 |K'| <= n 2^-53 c_h per entry: one flat bound per entry for both
    const double b = (256. + n) * 1.1102230246251565e-16 * ch;
    // probes
    const DenseMatrix<double> Z = K->model_probes(m, 7);
    if (Z.rows() != (std::size_t)n || Z.cols() != (std::size_t)m) return fail("model_probes: shape");
    bool differ = false;
    const DenseMatrix<double> Z8 = K->model_probes(m, 8);
    for (int c = 0; c < m; c++) for (int i = 0; i < n; i++) {
      if (std::abs(Z(i, c)) != 1.) return fail("model_probes: an entry that is not +-1");
      differ = differ || Z(i, c) != Z8(i, c);
    }
    if (!differ) return fail("model_probes: the seed does nothing");
    const kernel::LmlGradient G = K->log_marginal_likelihood_gradient(Z), G2 = K->log_marginal_likelihood_gradient(m, 7);
    if (G.dh != G2.dh || G.dlambda != G2.dlambda || G.th != G2.th || G.tl != G2.tl) return fail("seeded and explicit gradients differ");
    if ((int)G.th.size() != m || (int)G.tl.size() != m) return fail("per-probe values: count");
    // quad terms
    long double aa = 0.L, aka = 0.L, a1 = 0.L;
    for (int j = 0; j < n; j++) {
      aa += (long double)w(j, 0) * w(j, 0);
      a1 += std::abs(w(j, 0));
      for (int i = 0; i < n; i++) aka += (long double)w(i, 0) * Kp[i + (size_t)j * n] * w(j, 0);
    }
    const double bq = (double)(0.5L * a1 * a1) * b + 1e-13 * std::abs((double)aka);
    std::cout << tag << "quad_h " << G.quad_h << " dense " << (double)(0.5L * aka) << " bound " << bq << ", quad_lambda " << G.quad_lambda << std::endl;
    if (std::abs(G.quad_h - (double)(0.5L * aka)) > bq) return fail("quad_h");
    if (std::abs(G.quad_lambda - (double)(0.5L * aa)) > 1e-14 * (double)aa) return fail("quad_lambda");
    // per-probe values of the first probes: forward error of both solves (2e-12 cond ||s|| ||g||) + sum |s| b ||z||_1
    double worst = 0.;
    for (int c = 0; c < full; c++) {
      std::vector<double> s(n), gz(n, 0.), z(n);
      for (int i = 0; i < n; i++) z[i] = s[i] = Z(i, c);
      D.solve(s, false);
      for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) gz[i] += Kp[i + (size_t)j * n] * z[j];
      double th = 0., tl = 0., s1 = 0.;
      for (int i = 0; i < n; i++) { th += s[i] * gz[i]; tl += s[i] * z[i]; s1 += std::abs(s[i]); }
      const double bh = 2e-12 * cond * norm2(s) * norm2(gz) + s1 * b * n, bl = 2e-12 * cond * norm2(s) * norm2(z);
      worst = std::max(worst, std::max(std::abs(G.th[c] - th) / bh, std::abs(G.tl[c] - tl) / bl));
      if (std::abs(G.th[c] - th) > bh || std::abs(G.tl[c] - tl) > bl) {
        std::cout << tag << "probe " << c << ": th " << G.th[c] << " dense " << th << " bound " << bh << ", tl " << G.tl[c] << " dense " << tl << " bound " << bl << std::endl;
        return fail("per-probe values");
      }
    }
    std::cout << tag << "largest per-probe error / bound " << worst << " (cond " << cond << ")" << std::endl;
    // assembly
    double sh = 0., sl = 0.;
    for (int c = 0; c < m; c++) { sh += G.th[c]; sl += G.tl[c]; }
    if (std::abs(G.trace_h - sh / m) > 1e-13 * std::abs(sh / m) || std::abs(G.trace_lambda - sl / m) > 1e-13 * std::abs(sl / m)) return fail("trace means");
    if (std::abs(G.dh - (G.quad_h - 0.5 * G.trace_h)) > 1e-15 * (std::abs(G.quad_h) + std::abs(G.trace_h)) ||
        std::abs(G.dlambda - (G.quad_lambda - 0.5 * G.trace_lambda)) > 1e-15 * (std::abs(G.quad_lambda) + std::abs(G.trace_lambda)))
      return fail("assembly of the gradient");
    // tl_k = z^T H^-1 z is positive for a definite H, and the estimate of tr(H^-1) lies between n / sigma_max and n / sigma_min
    if (!(G.trace_lambda > n / D.normF && G.trace_lambda < n * D.inv2 * 1.1)) return fail("trace_lambda outside the spectrum's range");
    // residual against the exact kernel matrix
    {
      long double num = 0.L, den = 0.L;
      for (int i = 0; i < n; i++) {
        long double r = y[i] - (long double)lambda * w(i, 0);
        for (int j = 0; j < n; j++) r -= (long double)Ke[i + (size_t)j * n] * w(j, 0);
        num += r * r;
        den += (long double)y[i] * y[i];
      }
      const double ref = (double)std::sqrt(num / den), got = K->model_residual();
      // a row of the product: entries within 512 * 2^-53 of theirs, n roundings of the sum, against ||alpha||_1
      const double br = (512. + n) * 1.1102230246251565e-16 * (double)a1 * std::sqrt((double)n) / std::sqrt((double)den);
      std::cout << tag << "residual " << got << " dense " << ref << " bound " << br << std::endl;
      if (std::abs(got - ref) > br) return fail("model_residual");
      if (!(ref > 1e3 * br)) return fail("the residual case proves nothing");
    }
    // refusals leave the model alone
    if (!throws([&] { K->log_marginal_likelihood_gradient(0, 1); }) || !throws([&] { K->model_probes(0, 1); })) return fail("m = 0 accepted");
    if (!throws([&] { K->log_marginal_likelihood_gradient(DenseMatrix<double>(n - 1, 3)); })) return fail("a probe block of the wrong height accepted");
    if (!throws([&] { K->log_marginal_likelihood_gradient(DenseMatrix<double>(n, 0)); })) return fail("an empty probe block accepted");
    if (K->logabsdet() != ld) return fail("the gradient disturbed the kept model");
    const kernel::LmlGradient G3 = K->log_marginal_likelihood_gradient(Z);
    if (G3.dh != G.dh || G3.th != G.th) return fail("two gradient calls differ");
    // after a new lambda the gradient follows
    K->model_set_lambda(0.5);
    const kernel::LmlGradient G4 = K->log_marginal_likelihood_gradient(Z);
    if (G4.dlambda == G.dlambda || !(G4.trace_lambda > G.trace_lambda)) return fail("the gradient did not follow set_lambda");
    K->keep_model(false);
    if (!throws([&] { K->log_marginal_likelihood_gradient(Z); })) return fail("keep_model(false) kept the model");
  }
  {   // ANOVA: a model, but no derivative and no product
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    auto K = kernel::create_kernel<double>(kernel::KernelType::ANOVA, Xc, h, lambda, 2);
    K->keep_model(true);
    K->fit_HSS(y, opts);
    const double ld = K->logabsdet();
    if (!throws([&] { K->log_marginal_likelihood_gradient(5, 1); }) || !throws([&] { K->model_residual(); })) return fail("an ANOVA gradient");
    if (K->logabsdet() != ld) return fail("a refused call disturbed the ANOVA model");
  }
  {   // a user-defined kernel keeps no model
    DenseMatrix<double> Xc(X);
    std::vector<double> y(labels);
    CauchyKernel K(Xc, h, lambda);
    K.keep_model(true);
    K.fit_HSS(y, opts);
    if (!throws([&] { K.log_marginal_likelihood_gradient(5, 1); }) || !throws([&] { K.model_residual(); })) return fail("a user-defined kernel answered");
  }
  std::cout << "# exiting" << std::endl;
  return 0;
}
