// The C interface of include/kernel/Kernel.h (reference: kernel/Kernel.cpp:43-180).
#include <functional>

#include "KernelModel.hpp"
#include "NeighborSearch.hpp"
#include "kernel/Kernel.h"

using namespace strumpack;
namespace {
using KernelD = kernel::Kernel<double>;
struct KernelRegression {
  int precision = 0;   // the tag of the handle: 0 = double (K, training, weights), 1 = float (Kf, trainingf, weightsf)
  std::unique_ptr<KernelD> K;
  DenseMatrix<double> training, weights;
  std::unique_ptr<kernel::Kernel<float>> Kf;
  DenseMatrix<float> trainingf, weightsf;
  float* caller_train = nullptr;   // the float caller's array: reordered in place by the fit
  bool any() const { return precision ? bool(Kf) : bool(K); }
  long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<int> nodes;   // node table of the last fit (6 ints per node)
  void keep_fit_info() {
    std::copy(kernel::last_fit_info(), kernel::last_fit_info() + 8, info);
    nodes = kernel::last_fit_nodes();
  }
};
void report(const std::exception& e) { std::cerr << "Operation failed: " << e.what() << std::endl; }

// The frame of an entry point: what f() returns, or `fail` after reporting what it threw.
template <class R, class F> R guarded(R fail, F&& f) { try { return f(); } catch (const std::exception& e) { report(e); return fail; } }
template <class F> int guarded(F&& f) { return guarded(1, f); }

KernelRegression* handle(STRUMPACKKernel K) { return static_cast<KernelRegression*>(K); }
// the kernel of a double / float handle, null for anything else
KernelD* double_of(STRUMPACKKernel K) { auto kr = handle(K); return kr && kr->precision == 0 ? kr->K.get() : nullptr; }
kernel::Kernel<float>* float_of(STRUMPACKKernel K) { auto kr = handle(K); return kr && kr->precision == 1 ? kr->Kf.get() : nullptr; }
// ... of a double handle with a built-in kernel: the ones that can keep a model
KernelD* builtin_of(STRUMPACKKernel K) { auto k = double_of(K); return k && k->device_type() >= 0 ? k : nullptr; }
// ---- the kept model (double handles, built-in kernels): every call returns non-zero, outputs untouched, without one
KernelD* model_of(STRUMPACKKernel K) { auto k = builtin_of(K); return k && k->has_model() ? k : nullptr; }
// f(k) on the kernel with the kept model of K (f: what is left of the preconditions, the call, then the outputs)
template <class F> int with_model(STRUMPACKKernel K, F&& f) { return guarded([&] { auto k = model_of(K); return k ? f(*k) : 1; }); }
// one number of the kept model / `count` stopwatch or counter values of its last call (exact: Gauss and Laplace only, where for
// an ANOVA kernel none of the calls that fill them exists)
int scalar_out(STRUMPACKKernel K, double* out, double (KernelD::*get)() const) {
  return with_model(K, [&](KernelD& k) { if (!out) return 1; const double v = (k.*get)(); *out = v; return 0; });
}
int array_out(STRUMPACKKernel K, double* out, const double* (KernelD::*get)() const, int count, bool exact = false) {
  return with_model(K, [&](KernelD& k) {
    if (!out || (exact && !kernel::exact_products(k))) return 1;
    std::copy((k.*get)(), (k.*get)() + count, out);
    return 0;
  });
}
HSS::HSSOptions<double> fit_options(int argc, char* argv[]) {
  HSS::HSSOptions<double> opts;   // (also the promoted float fit's options: tolerances do not pass through a float)
  opts.set_verbose(false);
  opts.set_clustering_algorithm(ClusteringAlgorithm::COBBLE);   // kernel/Kernel.cpp:82
  opts.set_from_command_line(argc, argv);
  return opts;
}
// info: 8 + 2 m doubles (include/kernel/Kernel.h)
void krylov_info_out(const kernel::KrylovInfo& I, double* info) {
  if (!info) return;
  const std::size_t m = I.its.size();
  info[0] = I.converged ? 1. : 0.; info[1] = I.iterations; info[2] = (double)I.products; info[3] = (double)I.solves; info[4] = (double)I.cycles;
  info[5] = m ? *std::max_element(I.residual0.begin(), I.residual0.end()) : 0.;
  info[6] = m ? *std::max_element(I.residual.begin(), I.residual.end()) : 0.;
  info[7] = (double)m;
  std::copy(I.residual.begin(), I.residual.end(), info + 8);
  for (std::size_t c = 0; c < m; c++) info[8 + m + c] = I.its[c];
}
ClusteringAlgorithm clustering_algorithm(int algo) {
  static const ClusteringAlgorithm algos[] = {ClusteringAlgorithm::NATURAL, ClusteringAlgorithm::TWO_MEANS, ClusteringAlgorithm::KD_TREE,
                                              ClusteringAlgorithm::PCA, ClusteringAlgorithm::COBBLE};
  if (algo < 0 || algo > 4) throw std::invalid_argument("clustering algorithm out of range");
  return algos[algo];
}
// the leaf sizes of the tree, left to right, as far as cap allows; returns the number of leaves
int leaf_sizes_out(const structured::ClusterTree& tree, int* leaf_sizes, int cap) {
  int c = 0;
  std::function<void(const structured::ClusterTree&)> walk = [&](const structured::ClusterTree& nd) {
    if (nd.c.empty()) { if (c < cap) leaf_sizes[c] = nd.size; c++; }
    else for (auto& ch : nd.c) walk(ch);
  };
  walk(tree);
  return c;
}
}  // namespace

extern "C" {

STRUMPACKKernel STRUMPACK_create_kernel_double(int n, int d, double* train, double h, double lambda, int p, int type) {
  return guarded<STRUMPACKKernel>(nullptr, [&]() -> STRUMPACKKernel {
    auto kr = new KernelRegression();
    kr->training = DenseMatrix<double>(d, n, train, d);
    kr->K = kernel::make_kernel<double>(type, kr->training, h, lambda, p);
    if (!kr->K) std::cout << "ERROR: Kernel type not recognized!" << std::endl;
    return kr;
  });
}
void STRUMPACK_destroy_kernel_double(STRUMPACKKernel K) { delete handle(K); }

void STRUMPACK_kernel_fit_HSS_double(STRUMPACKKernel K, double* labels, int argc, char* argv[]) {
  guarded([&] {
    auto k = double_of(K);
    if (!k) throw std::invalid_argument("no kernel");
    std::vector<double> vl(labels, labels + k->n());
    handle(K)->weights = k->fit_HSS(vl, fit_options(argc, argv));
    handle(K)->keep_fit_info();
    return 0;
  });
}
void STRUMPACK_kernel_predict_double(STRUMPACKKernel K, int m, double* test, double* prediction) {
  guarded([&] {
    auto k = double_of(K);
    if (!k) throw std::invalid_argument("no kernel");
    DenseMatrix<double> t(k->d(), m, test, k->d());
    auto pred = k->predict(t, handle(K)->weights);
    std::copy(pred.begin(), pred.end(), prediction);
    return 0;
  });
}

STRUMPACKKernel STRUMPACK_create_kernel_float(int n, int d, float* train, float h, float lambda, int p, int type) {
  return guarded<STRUMPACKKernel>(nullptr, [&]() -> STRUMPACKKernel {
    auto kr = new KernelRegression();
    kr->precision = 1;
    kr->caller_train = train;
    kr->trainingf = DenseMatrix<float>(d, n, train, d);
    kr->Kf = kernel::make_kernel<float>(type, kr->trainingf, h, lambda, p);
    if (!kr->Kf) std::cout << "ERROR: Kernel type not recognized!" << std::endl;
    return kr;
  });
}
void STRUMPACK_destroy_kernel_float(STRUMPACKKernel K) { delete handle(K); }

void STRUMPACK_kernel_fit_HSS_float(STRUMPACKKernel K, float* labels, int argc, char* argv[]) {
  guarded([&] {
    auto k = float_of(K);
    if (!k) throw std::invalid_argument("no float kernel");
    auto kr = handle(K);
    const std::size_t n = k->n(), d = k->d();
    std::vector<float> vl(labels, labels + n);
    kr->weightsf = k->fit_HSS(vl, fit_options(argc, argv));
    // the cluster order reaches the caller's arrays, as in the reference (which works on them in place)
    std::copy(vl.begin(), vl.end(), labels);
    if (kr->caller_train) std::copy(kr->trainingf.data(), kr->trainingf.data() + n * d, kr->caller_train);
    kr->keep_fit_info();
    return 0;
  });
}
void STRUMPACK_kernel_predict_float(STRUMPACKKernel K, int m, float* test, float* prediction) {
  guarded([&] {
    auto k = float_of(K);
    if (!k) throw std::invalid_argument("no float kernel");
    DenseMatrix<float> t(k->d(), m, test, k->d());
    auto pred = k->predict(t);
    std::copy(pred.begin(), pred.end(), prediction);
    return 0;
  });
}
int SPX_kernel_predict_device_float(STRUMPACKKernel K, int m, const float* dtest, float* dpred) {
  return guarded([&] { auto k = float_of(K); return k ? k->predict_device(m, dtest, dpred) : 1; });
}
int SPX_kernel_predict_stats(STRUMPACKKernel K, long long* out) {
  auto k = float_of(K);
  if (!k) return 1;
  std::copy(k->predict_stats(), k->predict_stats() + 6, out);
  return 0;
}
int SPX_approximate_neighbors(int n, int d, const double* data, int iterations, int k, int* ann, double* scores) {
  return guarded([&] {
    DenseMatrix<double> p(d, n, data, d);
    DenseMatrix<std::uint32_t> nb;
    DenseMatrix<double> sc;
    find_approximate_neighbors(p, iterations, k, nb, sc);
    for (size_t i = 0; i < (size_t)k * n; i++) { ann[i] = (int)nb.data()[i]; if (scores) scores[i] = sc.data()[i]; }
    return 0;
  });
}
int SPX_kernel_set_neighbors(STRUMPACKKernel K, int k, const int* ann) {
  auto kr = handle(K);
  if (!kr || !kr->any()) return 1;
  if (kr->precision) kr->Kf->set_neighbors(ann, k);
  else kr->K->set_neighbors(ann, k);
  return 0;
}
int SPX_kernel_node_info(STRUMPACKKernel K, int* out, int cap) {
  auto kr = handle(K);
  if (!kr) return -1;
  int c = (int)kr->nodes.size() / 6;
  std::copy(kr->nodes.begin(), kr->nodes.begin() + 6 * std::min(c, cap), out);
  return c;
}
int SPX_kernel_fit_info(STRUMPACKKernel K, long long* out) {
  auto kr = handle(K);
  if (!kr) return 1;
  std::copy(kr->info, kr->info + 8, out);
  return 0;
}
int SPX_kernel_permutation(STRUMPACKKernel K, int* perm) {
  auto kr = handle(K);
  if (!kr || !kr->any()) return 1;
  const std::vector<int>& pm = kr->precision ? kr->Kf->permutation() : kr->K->permutation();
  std::copy(pm.begin(), pm.end(), perm);
  return 0;
}
int SPX_kernel_weights(STRUMPACKKernel K, double* w) {
  auto kr = handle(K);
  if (kr && kr->precision) {   // the float weights, widened
    if (kr->weightsf.rows() == 0) return 1;
    for (std::size_t i = 0; i < kr->weightsf.rows(); i++) w[i] = (double)kr->weightsf(i, 0);
    return 0;
  }
  if (!kr || kr->weights.rows() == 0) return 1;
  std::copy(kr->weights.data(), kr->weights.data() + kr->weights.rows(), w);
  return 0;
}

// ---- the kept model ----
int SPX_kernel_keep_model(STRUMPACKKernel K, int keep) {
  return guarded([&] { auto k = builtin_of(K); if (!k) return 1; k->keep_model(keep != 0); return 0; });
}
int SPX_kernel_logabsdet(STRUMPACKKernel K, double* out) { return scalar_out(K, out, &KernelD::logabsdet); }
int SPX_kernel_log_marginal_likelihood(STRUMPACKKernel K, double* out) { return scalar_out(K, out, &KernelD::log_marginal_likelihood); }
int SPX_kernel_model_residual(STRUMPACKKernel K, double* out) { return scalar_out(K, out, &KernelD::model_residual); }
int SPX_kernel_variance_ms(STRUMPACKKernel K, double* out) { return array_out(K, out, &KernelD::variance_ms, 3); }
int SPX_kernel_gradient_ms(STRUMPACKKernel K, double* out) { return array_out(K, out, &KernelD::gradient_ms, 3); }
int SPX_kernel_krylov_ms(STRUMPACKKernel K, double out[3]) { return array_out(K, out, &KernelD::krylov_ms, 3, true); }
int SPX_kernel_krylov_stats(STRUMPACKKernel K, double out[6]) { return array_out(K, out, &KernelD::krylov_stats, 6, true); }

int SPX_kernel_predict_variance_double(STRUMPACKKernel K, int m, const double* test, double* var) {
  return with_model(K, [&](KernelD& k) {
    if (m < 0 || (m > 0 && (!test || !var))) return 1;
    DenseMatrix<double> t(k.d(), m, test, k.d());
    const std::vector<double> v = k.predict_variance(t);
    std::copy(v.begin(), v.end(), var);
    return 0;
  });
}
int SPX_kernel_model_set_lambda(STRUMPACKKernel K, double lambda) {
  return with_model(K, [&](KernelD& k) { handle(K)->weights = k.model_set_lambda(lambda); return 0; });
}
int SPX_kernel_model_write(STRUMPACKKernel K, const char* path) {
  return with_model(K, [&](KernelD& k) { if (!path) return 1; k.model_write(path); return 0; });
}
int SPX_kernel_model_labels(STRUMPACKKernel K, double* y) {
  return with_model(K, [&](KernelD& k) { if (!y) return 1; std::copy(k.model_labels().begin(), k.model_labels().end(), y); return 0; });
}
int SPX_kernel_model_points(STRUMPACKKernel K, double* x) {
  return with_model(K, [&](KernelD& k) {
    if (!x) return 1;
    for (std::size_t i = 0; i < k.n(); i++) std::copy(k.data().ptr(0, i), k.data().ptr(0, i) + k.d(), x + i * k.d());
    return 0;
  });
}

int SPX_kernel_lml_gradient(STRUMPACKKernel K, int m, const double* Z, unsigned long long seed, double grad[2], double* terms) {
  return with_model(K, [&](KernelD& k) {
    if (m < 1 || !grad) return 1;
    const kernel::LmlGradient g = Z ? k.log_marginal_likelihood_gradient(DenseMatrix<double>(k.n(), m, Z, k.n()))
                                    : k.log_marginal_likelihood_gradient(m, seed);
    grad[0] = g.dh;
    grad[1] = g.dlambda;
    if (terms) {
      terms[0] = g.quad_h; terms[1] = g.quad_lambda; terms[2] = g.trace_h; terms[3] = g.trace_lambda;
      std::copy(g.th.begin(), g.th.end(), terms + 4);
      std::copy(g.tl.begin(), g.tl.end(), terms + 4 + m);
    }
    return 0;
  });
}
int SPX_kernel_lml_gradient_coords(STRUMPACKKernel K, int m, const double* Z, unsigned long long seed, double* grad, double* terms) {
  return with_model(K, [&](KernelD& k) {
    if (m < 1 || !grad) return 1;
    const kernel::LmlGradientCoords g = Z ? k.log_marginal_likelihood_gradient_coords(DenseMatrix<double>(k.n(), m, Z, k.n()))
                                          : k.log_marginal_likelihood_gradient_coords(m, seed);
    const std::size_t dim = k.d();
    std::copy(g.dtheta.begin(), g.dtheta.end(), grad);
    if (terms) {
      std::copy(g.quad.begin(), g.quad.end(), terms);
      std::copy(g.trace.begin(), g.trace.end(), terms + dim);
      std::copy(g.tc.begin(), g.tc.end(), terms + 2 * dim);
    }
    return 0;
  });
}
int SPX_kernel_model_probes(STRUMPACKKernel K, int m, unsigned long long seed, double* Z) {
  return with_model(K, [&](KernelD& k) {
    if (m < 1 || !Z) return 1;
    const DenseMatrix<double> P = k.model_probes(m, seed);
    for (int c = 0; c < m; c++) std::copy(P.ptr(0, c), P.ptr(0, c) + k.n(), Z + (size_t)c * k.n());
    return 0;
  });
}

// ---- solves with the exact kernel matrix ----
int SPX_kernel_model_refine(STRUMPACKKernel K, double rtol, int maxit, int restart, double* info) {
  return with_model(K, [&](KernelD& k) {
    const kernel::KrylovInfo I = k.model_refine(rtol, maxit, restart);
    handle(K)->weights = k.model_weights();
    krylov_info_out(I, info);
    return 0;
  });
}
int SPX_kernel_model_solve(STRUMPACKKernel K, int m, const double* B, int ldb, double* X, int ldx, double rtol, int maxit, int restart,
                           double* info) {
  return with_model(K, [&](KernelD& k) {
    if (m < 0 || (m > 0 && (!B || !X || ldb < (int)k.n() || ldx < (int)k.n()))) return 1;
    kernel::KrylovInfo I;
    const DenseMatrix<double> S = k.model_solve(DenseMatrix<double>(k.n(), m, B, ldb), &I, rtol, maxit, restart);
    for (int c = 0; c < m; c++) std::copy(S.ptr(0, c), S.ptr(0, c) + k.n(), X + (size_t)c * ldx);
    krylov_info_out(I, info);
    return 0;
  });
}
int SPX_kernel_predict_variance_exact_double(STRUMPACKKernel K, int m, const double* test, double* var, double rtol, int maxit, int restart,
                                             double* info) {
  return with_model(K, [&](KernelD& k) {
    if (m < 0 || (m > 0 && (!test || !var))) return 1;
    kernel::KrylovInfo I;
    DenseMatrix<double> t(k.d(), m, test, k.d());
    const std::vector<double> v = k.predict_variance_exact(t, &I, rtol, maxit, restart);
    std::copy(v.begin(), v.end(), var);
    krylov_info_out(I, info);
    return 0;
  });
}
// ---- gradients in the test points ----
int SPX_kernel_predict_gradient_double(STRUMPACKKernel K, int m, const double* test, double* grad) {
  return guarded([&] {
    auto k = builtin_of(K);
    if (!k || k->device_type() > 1 || k->d() > 64 || handle(K)->weights.rows() != k->n()) return 1;
    if (m < 0 || (m > 0 && (!test || !grad))) return 1;
    const DenseMatrix<double> g = k->predict_gradient(DenseMatrix<double>(k->d(), m, test, k->d()), handle(K)->weights);
    std::copy(g.data(), g.data() + k->d() * (std::size_t)m, grad);
    return 0;
  });
}
int SPX_kernel_predict_variance_gradient_double(STRUMPACKKernel K, int m, const double* test, double* var, double* grad) {
  return with_model(K, [&](KernelD& k) {
    if (m < 0 || (m > 0 && (!test || !var || !grad))) return 1;
    DenseMatrix<double> g;
    const std::vector<double> v = k.predict_variance_gradient(DenseMatrix<double>(k.d(), m, test, k.d()), g);
    std::copy(v.begin(), v.end(), var);
    std::copy(g.data(), g.data() + k.d() * (std::size_t)m, grad);
    return 0;
  });
}
int SPX_kernel_predict_variance_gradient_exact_double(STRUMPACKKernel K, int m, const double* test, double* var, double* grad, double rtol,
                                                      int maxit, int restart, double* info) {
  return with_model(K, [&](KernelD& k) {
    if (m < 0 || (m > 0 && (!test || !var || !grad))) return 1;
    kernel::KrylovInfo I;
    DenseMatrix<double> g;
    const std::vector<double> v = k.predict_variance_gradient_exact(DenseMatrix<double>(k.d(), m, test, k.d()), g, &I, rtol, maxit, restart);
    std::copy(v.begin(), v.end(), var);
    std::copy(g.data(), g.data() + k.d() * (std::size_t)m, grad);
    krylov_info_out(I, info);
    return 0;
  });
}
// ---- the joint predictive covariance ----
int SPX_kernel_covariance_ms(STRUMPACKKernel K, double out[3]) { return array_out(K, out, &KernelD::covariance_ms, 3, true); }
int SPX_kernel_predict_covariance_double(STRUMPACKKernel K, int m, const double* test, double* cov, int ldc) {
  return with_model(K, [&](KernelD& k) {
    if (m < 0 || (m > 0 && (!test || !cov || ldc < m))) return 1;
    const DenseMatrix<double> c = k.predict_covariance(DenseMatrix<double>(k.d(), m, test, k.d()));
    for (int b = 0; b < m; b++) std::copy(c.ptr(0, b), c.ptr(0, b) + m, cov + (std::size_t)b * ldc);
    return 0;
  });
}
int SPX_kernel_predict_covariance_exact_double(STRUMPACKKernel K, int m, const double* test, double* cov, int ldc, double rtol, int maxit,
                                               int restart, double* info) {
  return with_model(K, [&](KernelD& k) {
    if (m < 0 || (m > 0 && (!test || !cov || ldc < m))) return 1;
    kernel::KrylovInfo I;
    const DenseMatrix<double> c = k.predict_covariance_exact(DenseMatrix<double>(k.d(), m, test, k.d()), &I, rtol, maxit, restart);
    for (int b = 0; b < m; b++) std::copy(c.ptr(0, b), c.ptr(0, b) + m, cov + (std::size_t)b * ldc);
    krylov_info_out(I, info);
    return 0;
  });
}
int SPX_kernel_set_krylov_inner(STRUMPACKKernel K, int precision, double inner_rtol) {
  return guarded([&] {
    auto k = builtin_of(K);
    if (!k || (precision != 0 && precision != 1) || std::isnan(inner_rtol)) return 1;
    k->krylov_inner(precision ? kernel::KrylovInner::FP32 : kernel::KrylovInner::FP64,
                    inner_rtol <= 0. ? kernel::KRYLOV_INNER_RTOL_DEFAULT : inner_rtol);
    return 0;
  });
}
int SPX_kernel_krylov_inner(STRUMPACKKernel K, int* precision, double* inner_rtol) {
  auto k = builtin_of(K);
  if (!k) return 1;
  if (precision) *precision = k->krylov_inner() == kernel::KrylovInner::FP32 ? 1 : 0;
  if (inner_rtol) *inner_rtol = k->krylov_inner_rtol();
  return 0;
}

int SPX_clustering(int n, int d, double* data, int algo, int leaf_size, int* perm, int* leaf_sizes, int cap) {
  return guarded(-1, [&] {
    DenseMatrix<double> p(d, n, data, d);
    std::vector<int> pm;
    auto t = binary_tree_clustering(clustering_algorithm(algo), p, pm, leaf_size);
    std::copy(p.data(), p.data() + (size_t)d * n, data);
    std::copy(pm.begin(), pm.end(), perm);
    return leaf_sizes_out(t, leaf_sizes, cap);
  });
}

int SPX_clustering_device(int n, int d, double* data, int algo, int leaf_size, int* perm, int* leaf_sizes, int cap, int* status) {
  return guarded(-1, [&] {
    DenseMatrix<double> p(d, n, data, d);
    std::vector<int> pm;
    structured::ClusterTree t(0);
    const int st = binary_tree_clustering_device(clustering_algorithm(algo), p, pm, (std::size_t)leaf_size, device_from_env(), t);
    if (status) *status = st;
    if (st) return 0;
    std::copy(p.data(), p.data() + (size_t)d * n, data);
    std::copy(pm.begin(), pm.end(), perm);
    return leaf_sizes_out(t, leaf_sizes, cap);
  });
}

}  // extern "C"
