// Kernel<double>::fit_HSS / predict (reference: kernel/KernelRegression.hpp:56-123), the kept model and its predictive variance,
// and the gradients of both predictions in the test points.  The gradients of the likelihood are in KernelGradient.cpp, the
// solves with the exact kernel matrix in KernelKrylov.cpp, Kernel<float> in KernelFloat.cpp and the C interface of
// include/kernel/Kernel.h in KernelC.cpp.
#include <chrono>
#include <optional>

#include "KernelModel.hpp"

namespace strumpack {
namespace kernel {

namespace {
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct FitInfo {
  long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
thread_local FitInfo last_fit;
thread_local std::vector<int> last_nodes;
}  // namespace

Kernel<double>::Kernel(DenseM_t& data, scalar_t lambda) : data_(data), lambda_(lambda) {}
Kernel<double>::~Kernel() = default;
void Kernel<double>::keep_model(bool keep) {
  keep_model_ = keep;
  if (!keep) model_.reset();
}
bool Kernel<double>::has_model() const { return bool(model_); }
const Kernel<double>::Model& Kernel<double>::model(const char* what) const {
  if (!model_) throw std::logic_error(std::string(what) + ": no kept model (keep_model(true) before fit_HSS; built-in kernels only)");
  return *model_;
}
double Kernel<double>::logabsdet() const { return model("logabsdet").H.logabsdet(); }
const std::vector<double>& Kernel<double>::model_labels() const { return model("model_labels").labels; }
const DenseMatrix<double>& Kernel<double>::model_weights() const { return model("model_weights").weights; }
void Kernel<double>::model_write(const std::string& path) const { model("model_write").H.write(path); }

double Kernel<double>::log_marginal_likelihood() const {
  const Model& M = model("log_marginal_likelihood");
  const double ld = M.H.logabsdet();
  long double ya = 0.L;
  for (std::size_t i = 0; i < M.labels.size(); i++) ya += (long double)M.labels[i] * (long double)M.weights(i, 0);
  const long double two_pi = 6.283185307179586476925286766559L;
  return (double)(-0.5L * ya - 0.5L * (long double)ld - 0.5L * (long double)M.labels.size() * std::log(two_pi));
}

DenseMatrix<double> Kernel<double>::model_set_lambda(double lambda) {
  model("model_set_lambda");
  Model& M = *model_;
  M.H.shift(lambda - lambda_);
  lambda_ = lambda;
  M.H.factor();
  DenseMatrix<double> w(n(), 1, M.labels.data(), n());
  M.H.solve(w);
  M.weights = w;
  return w;
}

std::vector<double> Kernel<double>::predict_variance(const DenseMatrix<double>& test) const {
  const Model& M = model("predict_variance");
  if (test.rows() != d()) throw std::invalid_argument("predict_variance: test points have the wrong dimension");
  return variance_chunks(M, test, nullptr, 0., 0, 0, nullptr);
}

void Kernel<double>::require_point_gradient(const char* what) const {
  if (device_type() != 0 && device_type() != 1) throw std::invalid_argument(std::string(what) + ": Gauss and Laplace kernels only");
  if (d() > 64) throw std::invalid_argument(std::string(what) + ": at most 64 coordinates");
}

std::vector<double> Kernel<double>::predict_variance_gradient(const DenseMatrix<double>& test, DenseMatrix<double>& grad) const {
  const Model& M = model("predict_variance_gradient");
  require_point_gradient("predict_variance_gradient");
  if (test.rows() != d()) throw std::invalid_argument("predict_variance_gradient: test points have the wrong dimension");
  return variance_chunks(M, test, nullptr, 0., 0, 0, nullptr, &grad);
}

std::vector<double> Kernel<double>::variance_chunks(const Model& M, const DenseMatrix<double>& test, KrylovWork* ws, double rtol, int maxit, int restart,
                                                    KrylovInfo* info, DenseMatrix<double>* grad) const {
  const int m = int(test.cols()), dim = int(d()), CH = 64;
  const long long nn = (long long)n();
  std::vector<double> var(m, 0.);
  var_ms_[0] = var_ms_[1] = var_ms_[2] = 0.;
  if (grad) *grad = DenseMatrix<double>(dim, m);
  if (m == 0) return var;
  hssk_ctx* ctx = M.ctx();
  std::optional<PoolBuf> bG;   // (only where a gradient is asked for: the variance calls acquire what they always did)
  if (grad) bG.emplace(ctx, sizeof(double) * dim * m);
  double* dG = grad ? (double*)bG->p : nullptr;
  PoolBuf bT(ctx, sizeof(double) * dim * m), bK(ctx, sizeof(double) * nn * CH), bD(ctx, sizeof(double) * CH * CH), bP(ctx, sizeof(double) * m);
  double *dT = (double*)bT.p, *dK = (double*)bK.p, *dD = (double*)bD.p, *dP = (double*)bP.p;
  ckk(hssk_memcpy2d_h2d(ctx, dT, sizeof(double) * dim, test.data(), sizeof(double) * test.ld(), sizeof(double) * dim, m));
  std::vector<double> ktt(m, 0.), quad(m, 0.);
  const hssk_kernel_spec spec = kept_spec(*this, M.dX, 0.);
  for (int c0 = 0; c0 < m; c0 += CH) {
    const int mc = std::min(CH, m - c0);
    const double* dTc = dT + (size_t)c0 * dim;
    watched(ctx, 1, [&] { ckk(hssk_kernel_cross(ctx, &spec, dTc, mc, dK, nn)); });
    // k(t_c, t_c) by the same pair function: the diagonal of the chunk's own kernel block
    const hssk_kernel_spec self{dTc, (long long)mc, dim, device_type(), degree(), width(), 0.};
    ckk(hssk_kernel_cross(ctx, &self, dTc, mc, dD, mc));
    ckk(hssk_memcpy2d_d2h(ctx, ktt.data() + c0, sizeof(double), dD, sizeof(double) * (mc + 1), sizeof(double), mc));
    if (ws) ckk(hssk_memcpy_d2d(ctx, ws->B, dK, (long long)sizeof(double) * nn * mc));   // (the right-hand sides of the exact solve)
    watched(ctx, 2, [&] { M.H.solve_device(mc, dK, nn); });
    if (ws) {   // from H^-1 k on: the exact solve of the chunk's columns
      info->solves++;
      krylov_block(M, *ws, mc, dK, ws->B, rtol, maxit, restart, *info);
    }
    watched(ctx, 3, [&] { ckk(hssk_kernel_predict_cols(ctx, &spec, dK, nn, dTc, mc, dP + c0)); });
    // dK holds V = H^-1 k (or its refinement): the gradient sum with a weight column per test point
    if (grad) ckk(hssk_kernel_predict_grad(ctx, &spec, dK, nn, dTc, mc, dG + (size_t)c0 * dim, dim, 0));
  }
  ckk(hssk_memcpy_d2h(ctx, quad.data(), dP, (long long)sizeof(double) * m));
  for (int w = 0; w < 3; w++) var_ms_[w] = hssk_watch_read_ms(ctx, w + 1, nullptr);
  for (int c = 0; c < m; c++) var[c] = ktt[c] - quad[c];
  if (grad) {
    ckk(hssk_memcpy_d2h(ctx, grad->data(), dG, (long long)sizeof(double) * dim * m));
    for (int c = 0; c < m; c++)
      for (int j = 0; j < dim; j++) (*grad)(j, c) *= -2.;
  }
  return var;
}

DenseMatrix<double> Kernel<double>::predict_covariance(const DenseMatrix<double>& test) const {
  const Model& M = model("predict_covariance");
  require_exact_products(*this, "predict_covariance");
  if (test.rows() != d()) throw std::invalid_argument("predict_covariance: test points have the wrong dimension");
  return covariance_chunks(M, test, nullptr, 0., 0, 0, nullptr);
}

// Stopwatches 8 / 9 / 10: cross blocks, solves, products (1 .. 3 are the variance loop's, 4 .. 7 those of the Krylov code this may
// run around).
DenseMatrix<double> Kernel<double>::covariance_chunks(const Model& M, const DenseMatrix<double>& test, KrylovWork* ws, double rtol, int maxit,
                                                      int restart, KrylovInfo* info) const {
  const int m = int(test.cols()), dim = int(d()), CH = 64;
  const long long nn = (long long)n();
  cov_ms_[0] = cov_ms_[1] = cov_ms_[2] = 0.;
  DenseMatrix<double> C(m, m);
  if (m == 0) return C;
  hssk_ctx* ctx = M.ctx();
  for (int w = 8; w <= 10; w++) hssk_watch_read_ms(ctx, w, nullptr);   // (what a call that threw left recorded is dropped)
  PoolBuf bT(ctx, sizeof(double) * dim * m), bK(ctx, sizeof(double) * nn * CH), bQ(ctx, sizeof(double) * m * m), bC(ctx, sizeof(double) * m * m);
  double *dT = (double*)bT.p, *dK = (double*)bK.p, *dQ = (double*)bQ.p, *dC = (double*)bC.p;
  ckk(hssk_memcpy2d_h2d(ctx, dT, sizeof(double) * dim, test.data(), sizeof(double) * test.ld(), sizeof(double) * dim, m));
  const hssk_kernel_spec spec = kept_spec(*this, M.dX, 0.);
  // k(T, T) by the same pair function: the test points as the point set
  const hssk_kernel_spec self{dT, (long long)m, dim, device_type(), degree(), width(), 0.};
  watched(ctx, 8, [&] { ckk(hssk_kernel_cross_split(ctx, &self, dT, m, dC, m, 0)); });
  for (int c0 = 0; c0 < m; c0 += CH) {
    const int mc = std::min(CH, m - c0);
    const double* dTc = dT + (size_t)c0 * dim;
    watched(ctx, 8, [&] { ckk(hssk_kernel_cross_split(ctx, &spec, dTc, mc, dK, nn, 0)); });
    if (ws) ckk(hssk_memcpy_d2d(ctx, ws->B, dK, (long long)sizeof(double) * nn * mc));   // (the right-hand sides of the exact solve)
    watched(ctx, 9, [&] { M.H.solve_device(mc, dK, nn); });
    if (ws) {   // from H^-1 k on: the exact solve of the chunk's columns
      info->solves++;
      krylov_block(M, *ws, mc, dK, ws->B, rtol, maxit, restart, *info);
    }
    // Q(:, chunk) = k(T, X) V: every test point against the chunk's solved columns
    watched(ctx, 10, [&] { ckk(hssk_kernel_cross_matmul(ctx, &spec, dT, m, dK, nn, mc, dQ + (size_t)c0 * m, m, 0)); });
  }
  DenseMatrix<double> Q(m, m);
  ckk(hssk_memcpy_d2h(ctx, Q.data(), dQ, (long long)sizeof(double) * m * m));
  ckk(hssk_memcpy_d2h(ctx, C.data(), dC, (long long)sizeof(double) * m * m));
  for (int w = 0; w < 3; w++) cov_ms_[w] = hssk_watch_read_ms(ctx, w + 8, nullptr);
  // one value per pair {a, b}, stored twice: exactly symmetric whatever H^-1 is
  for (int b = 0; b < m; b++)
    for (int a = b; a < m; a++) {
      const double v = C(a, b) - 0.5 * (Q(a, b) + Q(b, a));
      C(a, b) = v;
      C(b, a) = v;
    }
  return C;
}

DenseMatrix<double> Kernel<double>::fit_HSS(std::vector<double>& labels, const HSS::HSSOptions<double>& opts) {
  if (labels.size() != n()) throw std::invalid_argument("fit_HSS: one label per training point expected");
  model_.reset();   // (the model of an earlier fit goes before the new compression asks for memory)
  double t0 = now();
  if (opts.verbose()) std::cout << "# starting HSS compression..." << std::endl;
  HSS::HSSMatrix<double> H(*this, opts);
  // labels to the cluster order: new label i = old label perm[i] (lapmt, forward)
  {
    std::vector<double> old(labels);
    for (std::size_t i = 0; i < labels.size(); i++) labels[i] = old[perm_[i] - 1];
  }
  double t1 = now();
  if (opts.verbose()) {
    std::cout << "# HSS compression time = " << t1 - t0 << std::endl;
    if (H.is_compressed())
      std::cout << "# created HSS matrix of dimension " << H.rows() << " x " << H.cols() << " with " << H.levels() << " levels" << std::endl
                << "# compression succeeded!" << std::endl;
    else std::cout << "# compression failed!!!" << std::endl;
    std::cout << "# rank(H) = " << H.rank() << std::endl << "# HSS memory(H) = " << H.memory() / 1e6 << " MB " << std::endl << std::endl
              << "# factorization start" << std::endl;
  }
  H.factor();
  double t2 = now();
  if (opts.verbose()) std::cout << "# factorization time = " << t2 - t1 << std::endl << "# solution start..." << std::endl;
  DenseMatrix<double> weights(n(), 1, labels.data(), n());
  H.solve(weights);
  double t3 = now();
  if (opts.verbose()) std::cout << "# solve time = " << t3 - t2 << std::endl;
  last_fit.v[0] = H.is_compressed(); last_fit.v[1] = (long long)H.levels(); last_fit.v[2] = (long long)H.rank();
  last_fit.v[3] = (long long)H.memory(); last_fit.v[4] = H.engine()->stats().d_final;
  last_nodes.assign(6 * (size_t)H.engine()->num_nodes(), 0);
  H.engine()->node_info(last_nodes.data());
  last_fit.v[5] = (long long)((t1 - t0) * 1e6); last_fit.v[6] = (long long)((t2 - t1) * 1e6); last_fit.v[7] = (long long)((t3 - t2) * 1e6);
  if (keep_model_ && device_type() >= 0 && n() > 0) {
    std::unique_ptr<Model> M(new Model(std::move(H)));
    M->labels = labels;
    M->weights = weights;
    M->bX = sizeof(double) * d() * n();
    M->dX = (double*)DevicePool::get().acquire(M->bX);
    if (!M->dX) throw std::runtime_error(hssk_last_error());
    ckk(hssk_memcpy2d_h2d(M->ctx(), M->dX, sizeof(double) * d(), data_.data(), sizeof(double) * data_.ld(), sizeof(double) * d(), (long long)n()));
    model_ = std::move(M);
  }
  return weights;
}

namespace {
// The scaffolding of predict and predict_gradient: a context and four buffers of the call's own (not the pool's) -- the points, the
// test points, the weights and `count` doubles of output --, then call(ctx, spec, weights, test points, output) and the output
// copied to `out`.  The buffers go first, then the context, on either way out.
template <class F>
void on_own_device(const Kernel<double>& K, const DenseMatrix<double>& test, const DenseMatrix<double>& weights, std::size_t count, double* out,
                   F&& call) {
  const int m = int(test.cols()), dim = int(K.d());
  const long long n = (long long)K.n();
  hssk_ctx* ctx = nullptr;
  ckk(hssk_ctx_create(&ctx, device_from_env()));
  struct Own { hssk_ctx* ctx; void* p[4]; ~Own() { for (void* q : p) hssk_free(q); hssk_ctx_destroy(ctx); } } own{ctx, {nullptr, nullptr, nullptr, nullptr}};
  auto dalloc = [&own](int i, long long bytes) { if (!(own.p[i] = hssk_malloc(bytes))) throw std::runtime_error(hssk_last_error()); return own.p[i]; };
  void* dX = dalloc(0, (long long)sizeof(double) * dim * n);
  void* dT = dalloc(1, (long long)sizeof(double) * dim * m);
  void* dw = dalloc(2, (long long)sizeof(double) * n);
  void* dp = dalloc(3, (long long)sizeof(double) * count);
  ckk(hssk_memcpy2d_h2d(ctx, dX, sizeof(double) * dim, K.data().data(), sizeof(double) * K.data().ld(), sizeof(double) * dim, n));
  ckk(hssk_memcpy2d_h2d(ctx, dT, sizeof(double) * dim, test.data(), sizeof(double) * test.ld(), sizeof(double) * dim, m));
  ckk(hssk_memcpy_h2d(ctx, dw, weights.data(), (long long)sizeof(double) * n));
  hssk_kernel_spec spec{(const double*)dX, n, dim, K.device_type(), K.degree(), K.width(), 0.};
  call(ctx, spec, (const double*)dw, (const double*)dT, (double*)dp);
  ckk(hssk_memcpy_d2h(ctx, out, dp, (long long)sizeof(double) * count));
  ckk(hssk_sync(ctx));
}
}  // namespace

std::vector<double> Kernel<double>::predict(const DenseMatrix<double>& test, const DenseMatrix<double>& weights) const {
  if (test.rows() != d()) throw std::invalid_argument("predict: test points have the wrong dimension");
  if (weights.rows() != n()) throw std::invalid_argument("predict: one weight per training point expected");
  const int m = int(test.cols());
  std::vector<double> prediction(m, 0.);
  if (m == 0) return prediction;
  if (device_type() < 0) {
    // a user-defined kernel function (only its virtual evaluation is known): the sums on the host
    for (int c = 0; c < m; c++) {
      double s = 0.;
      for (std::size_t r = 0; r < n(); r++) s += weights(r, 0) * eval_kernel_function(data_.ptr(0, r), test.ptr(0, c));
      prediction[c] = s;
    }
    return prediction;
  }
  on_own_device(*this, test, weights, m, prediction.data(), [&](hssk_ctx* ctx, const hssk_kernel_spec& spec, const double* dw, const double* dT, double* dp) {
    ckk(hssk_kernel_predict(ctx, &spec, dw, dT, m, dp));
  });
  return prediction;
}

DenseMatrix<double> Kernel<double>::predict_gradient(const DenseMatrix<double>& test, const DenseMatrix<double>& weights) const {
  require_point_gradient("predict_gradient");
  if (test.rows() != d()) throw std::invalid_argument("predict_gradient: test points have the wrong dimension");
  if (weights.rows() != n()) throw std::invalid_argument("predict_gradient: one weight per training point expected");
  const int m = int(test.cols()), dim = int(d());
  DenseMatrix<double> grad(dim, m);
  if (m == 0) return grad;
  on_own_device(*this, test, weights, (std::size_t)dim * m, grad.data(),
                [&](hssk_ctx* ctx, const hssk_kernel_spec& spec, const double* dw, const double* dT, double* dG) {
                  ckk(hssk_kernel_predict_grad(ctx, &spec, dw, 0, dT, m, dG, dim, 0));
                });
  return grad;
}

const long long* last_fit_info() { return last_fit.v; }
const std::vector<int>& last_fit_nodes() { return last_nodes; }

}  // namespace kernel
}  // namespace strumpack
