// kernel::Kernel<float> through create_kernel<float>: the promoted fit against the double class on the widened data (same
// permutation, float weights = the rounded double weights), the FP32 prediction against an FP64 sum on the host, the prediction
// from the resident model, and a user-defined float subclass (host prediction in float).   usage: test_float_kernel <n>
#include <cmath>
#include <iostream>
#include <random>
#include <vector>

#include "HSS/HSSMatrix.hpp"
#include "kernel/Kernel.hpp"
#include "kernel/KernelRegression.hpp"

using namespace strumpack;

// rational quadratic kernel in float: k(x, y) = 1 / (1 + |x - y|^2 / h^2)
class CauchyKernelF : public kernel::Kernel<float> {
 public:
  CauchyKernelF(DenseMatrix<float>& data, float h, float lambda) : Kernel<float>(data, lambda), h_(h) {}

 protected:
  float h_;
  float eval_kernel_function(const float* x, const float* y) const override {
    float s = 0.f;
    for (std::size_t k = 0; k < this->d(); k++) s += (x[k] - y[k]) * (x[k] - y[k]);
    return 1.f / (1.f + s / (h_ * h_));
  }
};

static int fail(const char* what) { std::cout << "ERROR: " << what << std::endl; return 1; }

int main(int argc, char* argv[]) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 300, d = 5, m = 70;
  std::mt19937 g(11);
  std::uniform_real_distribution<float> u(0.f, 1.f);
  DenseMatrix<float> X(d, n), T(d, m);
  for (int j = 0; j < n; j++) for (int i = 0; i < d; i++) X(i, j) = u(g);
  for (int j = 0; j < m; j++) for (int i = 0; i < d; i++) T(i, j) = u(g);
  std::vector<float> labels(n);
  for (int j = 0; j < n; j++) labels[j] = X(0, j) > 0.5f ? 1.f : -1.f;
  const float h = 0.75f, lambda = 2.f;
  HSS::HSSOptions<float> opts;
  opts.set_rel_tol(1e-4f); opts.set_abs_tol(1e-8f); opts.set_leaf_size(32);
  opts.set_clustering_algorithm(ClusteringAlgorithm::KD_TREE);
  opts.set_approximate_neighbors(64);
  HSS::HSSOptions<double> optsd;
  optsd.set_rel_tol(opts.rel_tol()); optsd.set_abs_tol(opts.abs_tol()); optsd.set_leaf_size(32);
  optsd.set_clustering_algorithm(ClusteringAlgorithm::KD_TREE);
  optsd.set_approximate_neighbors(64);
  const kernel::KernelType types[3] = {kernel::KernelType::GAUSS, kernel::KernelType::LAPLACE, kernel::KernelType::ANOVA};
  for (int t = 0; t < 3; t++) {
    DenseMatrix<float> Xf(X);
    std::vector<float> lf(labels);
    auto K = kernel::create_kernel<float>(types[t], Xf, h, lambda, 2);
    auto w = K->fit_HSS(lf, opts);
    // the double class on the widened points
    DenseMatrix<double> Xd(d, n);
    for (int j = 0; j < n; j++) for (int i = 0; i < d; i++) Xd(i, j) = (double)X(i, j);
    std::vector<double> ld(labels.begin(), labels.end());
    auto Kd = kernel::create_kernel<double>(types[t], Xd, (double)h, (double)lambda, 2);
    auto wd = Kd->fit_HSS(ld, optsd);
    if (K->permutation() != Kd->permutation()) return fail("permutation differs from the double class");
    for (int j = 0; j < n; j++) {
      if (w(j, 0) != (float)wd(j, 0)) return fail("float weights are not the rounded double weights");
      if (lf[j] != (float)ld[j]) return fail("labels are not in cluster order");
      for (int i = 0; i < d; i++)
        if ((double)Xf(i, j) != Xd(i, j) || Xf(i, j) != X(i, K->permutation()[j] - 1)) return fail("points are not in cluster order");
    }
    // prediction: caller-supplied weights, then the resident model; FP64 sums of the float kernel values as the yardstick
    auto p1 = K->predict(T, w);
    auto p2 = K->predict(T);
    const long long* st = K->predict_stats();
    if (st[5] != 1 || st[4] != 4LL * d * m) return fail("the resident prediction uploaded more than the test points");
    double worst = 0.;
    for (int c = 0; c < m; c++) {
      if (p1[c] != p2[c]) return fail("resident and caller-supplied weights disagree");
      double s = 0., sa = 0.;
      for (int r = 0; r < n; r++) {
        double q2 = 0., q1 = 0., e1 = 0., e2 = 0.;
        for (int i = 0; i < d; i++) {
          const double df = (double)Xf(i, r) - (double)T(i, c);
          q2 += df * df; q1 += std::abs(df);
          const double tt = std::exp(-df * df / (2. * h * h));
          e1 += tt; e2 += tt * tt;
        }
        const double k = t == 0 ? std::exp(-q2 / (2. * h * h)) : (t == 1 ? std::exp(-q1 / h) : 0.5 * (e1 * e1 - e2));
        s += (double)w(r, 0) * k; sa += std::abs((double)w(r, 0)) * std::abs(t == 2 ? 0.5 * (e1 * e1 + e2) : k);
      }
      worst = std::max(worst, std::abs(s - (double)p1[c]) / (sa + 1e-30));
    }
    std::cout << "# " << kernel::get_name(types[t]) << ": prediction error / sum |w| k = " << worst << ", tiles " << st[0] << " + " << st[1] << std::endl;
    if (worst > 1e-5) return fail("prediction");
  }
  {
    DenseMatrix<float> Xf(X);
    std::vector<float> lf(labels);
    CauchyKernelF K(Xf, h, lambda);
    auto w = K.fit_HSS(lf, opts);
    auto pred = K.predict(T, w);   // device_type() < 0: on the host, in float
    for (int c = 0; c < m; c++) {
      double s = 0.;
      for (int r = 0; r < n; r++) {
        double q = 0.;
        for (int k = 0; k < d; k++) q += ((double)Xf(k, r) - T(k, c)) * ((double)Xf(k, r) - T(k, c));
        s += (double)w(r, 0) / (1. + q / ((double)h * h));
      }
      if (std::abs(s - pred[c]) > 1e-3 * (1. + std::abs(s))) return fail("user-defined kernel: predict");
    }
    double num = 0, den = 0;
    for (int i = 0; i < n; i++) {
      double s = 0.;
      for (int j = 0; j < n; j++) s += (double)K.eval(i, j) * w(j, 0);
      num += (s - lf[i]) * (s - lf[i]); den += lf[i] * lf[i];
    }
    std::cout << "# user-defined float kernel: ||K w - y|| / ||y|| = " << std::sqrt(num / den) << std::endl;
    if (std::sqrt(num / den) > 1e-2) return fail("user-defined kernel: fit_HSS residual");
  }
  std::cout << "# exiting" << std::endl;
  return 0;
}
