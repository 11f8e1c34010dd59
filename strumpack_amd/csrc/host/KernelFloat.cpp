// Kernel<float>: promoted fit, native FP32 prediction from a model that stays in HBM.
#include "KernelModel.hpp"

namespace strumpack {
namespace kernel {

struct Kernel<float>::Resident {
  hssk_ctx* ctx = nullptr;
  float *dX = nullptr, *dw = nullptr;   // cluster-ordered points (d x n) and the weights of the last fit (device pool)
  size_t bX = 0, bw = 0;
  const float* src = nullptr;           // the host array dX is a copy of
  size_t n = 0, d = 0;
  bool have_w = false;
  // the context, created on first use
  hssk_ctx* context() { if (!ctx) ckk(hssk_ctx_create(&ctx, device_from_env())); return ctx; }
  // The points of `data` to a chunk of their own, and with them the weights w of a fit where there are any: both chunks are
  // acquired before either copy, a failed acquire drops everything, and what dX is a copy of is recorded after the copies.
  void upload_points(const DenseMatrix<float>& data, const float* w = nullptr) {
    const size_t nn = data.cols(), dd = data.rows();
    bX = sizeof(float) * dd * nn;
    dX = (float*)DevicePool::get().acquire(bX);
    if (w) { bw = sizeof(float) * nn; dw = (float*)DevicePool::get().acquire(bw); }
    if (!dX || (w && !dw)) { drop(); throw std::runtime_error(hssk_last_error()); }
    ckk(hssk_memcpy2d_h2d(ctx, dX, sizeof(float) * dd, data.data(), sizeof(float) * data.ld(), sizeof(float) * dd, (long long)nn));
    if (w) ckk(hssk_memcpy_h2d(ctx, dw, w, (long long)bw));
    src = data.data(); n = nn; d = dd;
    if (w) have_w = true;
  }
  void drop() {
    if (ctx && (dX || dw)) hssk_sync(ctx);
    if (dX) DevicePool::get().release(dX, bX);
    if (dw) DevicePool::get().release(dw, bw);
    dX = dw = nullptr; bX = bw = 0; src = nullptr; have_w = false;
  }
  ~Resident() {
    drop();
    if (ctx) hssk_ctx_destroy(ctx);
  }
};

namespace {
// a user-defined float kernel function in front of the FP64 front end (its points are exactly the widened floats)
class PromotedUserKernel : public Kernel<double> {
 public:
  PromotedUserKernel(DenseMatrix<double>& data, const Kernel<float>& f) : Kernel<double>(data, f.lambda()), f_(f) {}

 protected:
  const Kernel<float>& f_;
  double eval_kernel_function(const double* x, const double* y) const override {
    std::vector<float> a(d()), b(d());
    for (std::size_t i = 0; i < d(); i++) { a[i] = (float)x[i]; b[i] = (float)y[i]; }
    return (double)f_.kernel_function(a.data(), b.data());
  }
};
HSS::HSSOptions<double> widen(const HSS::HSSOptions<float>& o) {
  HSS::HSSOptions<double> w;
  w.set_rel_tol(o.rel_tol()); w.set_abs_tol(o.abs_tol()); w.set_leaf_size(o.leaf_size()); w.set_pivot_threshold(o.pivot_threshold());
  w.set_max_rank(o.max_rank()); w.set_verbose(o.verbose());
  w.set_d0(o.d0()); w.set_dd(o.dd()); w.set_p(o.p()); w.set_random_engine(o.random_engine());
  w.set_random_distribution(o.random_distribution()); w.set_compression_algorithm(o.compression_algorithm());
  w.set_compression_sketch(o.compression_sketch()); w.set_nnz0(o.nnz0()); w.set_nnz(o.nnz()); w.set_SJLT_algo(o.SJLT_algo());
  w.set_user_defined_random(o.user_defined_random()); w.set_symmetric_operand(o.symmetric_operand());
  w.set_factor_ahead(o.factor_ahead()); w.set_synchronized_compression(o.synchronized_compression()); w.set_log_ranks(o.log_ranks());
  w.set_clustering_algorithm(o.clustering_algorithm()); w.set_approximate_neighbors(o.approximate_neighbors());
  w.set_ann_iterations(o.ann_iterations()); w.set_neighbor_search(o.neighbor_search());
  return w;
}
}  // namespace

Kernel<float>::Kernel(DenseMatrix<float>& data, float lambda) : data_(data), lambda_(lambda) {}
Kernel<float>::~Kernel() = default;
bool Kernel<float>::fitted() const { return res_ && res_->have_w; }

DenseMatrix<float> Kernel<float>::fit_HSS(std::vector<float>& labels, const HSS::HSSOptions<float>& opts) { return fit_HSS(labels, widen(opts)); }

DenseMatrix<float> Kernel<float>::fit_HSS(std::vector<float>& labels, const HSS::HSSOptions<double>& opts) {
  if (labels.size() != n()) throw std::invalid_argument("fit_HSS: one label per training point expected");
  if (res_) res_->drop();
  const std::size_t nn = n(), dd = d();
  DenseMatrix<double> Xd(dd, nn);
  for (std::size_t i = 0; i < nn; i++)
    for (std::size_t j = 0; j < dd; j++) Xd(j, i) = (double)data_(j, i);
  std::unique_ptr<Kernel<double>> Kd = make_kernel<double>(device_type(), Xd, (double)width(), (double)lambda_, degree());
  if (!Kd) Kd.reset(new PromotedUserKernel(Xd, *this));
  if (neighbors()) Kd->set_neighbors(neighbors(), neighbor_count());
  std::vector<double> ld(labels.begin(), labels.end());
  DenseMatrix<double> wd = Kd->fit_HSS(ld, opts);
  // the cluster order back into the caller's arrays (narrowing widened floats is exact), the solution rounded once
  perm_ = Kd->permutation();
  for (std::size_t i = 0; i < nn; i++) {
    for (std::size_t j = 0; j < dd; j++) data_(j, i) = (float)Xd(j, i);
    labels[i] = (float)ld[i];
  }
  DenseMatrix<float> w(nn, 1);
  for (std::size_t i = 0; i < nn; i++) w(i, 0) = (float)wd(i, 0);
  if (device_type() >= 0 && nn > 0) {
    // the model stays in HBM: a prediction uploads test points only
    if (!res_) res_.reset(new Resident());
    res_->context();
    res_->upload_points(data_, w.data());
  }
  return w;
}

// test points: on the host (test_host, leading dimension ldt) or in HBM (test_dev); weights: on the host, or null = the resident
// ones; result to the host (out_host) or to HBM (out_dev)
void Kernel<float>::run_predict(int m, const float* test_host, int ldt, const float* test_dev, const float* weights_host,
                                float* out_host, float* out_dev) const {
  for (auto& v : pstats_) v = 0;
  if (m == 0) return;
  const std::size_t nn = n(), dd = d();
  if (!res_) res_.reset(new Resident());
  Resident& R = *res_;
  R.context();
  long long uploaded = 0;
  const bool resident = R.dX && R.src == data_.data() && R.n == nn && R.d == dd;
  if (!resident) {
    R.drop();
    R.upload_points(data_);
    uploaded += (long long)R.bX;
  }
  if (!weights_host && !R.have_w) throw std::invalid_argument("predict: no fit");
  std::unique_ptr<PoolBuf> wbuf, tbuf, pbuf;
  const float* dw = R.dw;
  if (weights_host) {
    wbuf.reset(new PoolBuf(R.ctx, sizeof(float) * nn));
    ckk(hssk_memcpy_h2d(R.ctx, wbuf->p, weights_host, (long long)(sizeof(float) * nn)));
    uploaded += (long long)(sizeof(float) * nn);
    dw = (const float*)wbuf->p;
  }
  const float* dT = test_dev;
  if (!dT) {
    tbuf.reset(new PoolBuf(R.ctx, sizeof(float) * dd * m));
    ckk(hssk_memcpy2d_h2d(R.ctx, tbuf->p, sizeof(float) * dd, test_host, sizeof(float) * ldt, sizeof(float) * dd, m));
    uploaded += (long long)(sizeof(float) * dd * m);
    dT = (const float*)tbuf->p;
  }
  float* dp = out_dev;
  if (!dp) { pbuf.reset(new PoolBuf(R.ctx, sizeof(float) * m)); dp = (float*)pbuf->p; }
  long long st[6];
  // (beyond 64 coordinates: the entry whose points pass through the LDS in chunks)
  ckk((dd <= 64 ? hssk_kernel_predict_f32 : hssk_kernel_predict_f32_wide)(R.ctx, R.dX, (long long)nn, (int)dd, device_type(), degree(),
                                                                          (double)width(), dw, dT, m, dp, st));
  if (out_host) ckk(hssk_memcpy_d2h(R.ctx, out_host, dp, (long long)(sizeof(float) * m)));
  ckk(hssk_sync(R.ctx));
  pstats_[0] = st[0]; pstats_[1] = st[1]; pstats_[2] = st[2]; pstats_[3] = st[3]; pstats_[4] = uploaded; pstats_[5] = resident ? 1 : 0;
}

std::vector<float> Kernel<float>::predict(const DenseMatrix<float>& test, const DenseMatrix<float>& weights) const {
  if (test.rows() != d()) throw std::invalid_argument("predict: test points have the wrong dimension");
  if (weights.rows() != n()) throw std::invalid_argument("predict: one weight per training point expected");
  const int m = int(test.cols());
  std::vector<float> prediction(m, 0.f);
  if (m == 0) return prediction;
  if (device_type() < 0) {
    // a user-defined kernel function: the sums on the host, in float
    for (int c = 0; c < m; c++) {
      float s = 0.f;
      for (std::size_t r = 0; r < n(); r++) s += weights(r, 0) * eval_kernel_function(data_.ptr(0, r), test.ptr(0, c));
      prediction[c] = s;
    }
    return prediction;
  }
  run_predict(m, test.data(), test.ld(), nullptr, weights.data(), prediction.data(), nullptr);
  return prediction;
}

std::vector<float> Kernel<float>::predict(const DenseMatrix<float>& test) const {
  if (test.rows() != d()) throw std::invalid_argument("predict: test points have the wrong dimension");
  if (!fitted()) throw std::invalid_argument("predict: no fit");
  std::vector<float> prediction(test.cols(), 0.f);
  run_predict(int(test.cols()), test.data(), test.ld(), nullptr, nullptr, prediction.data(), nullptr);
  return prediction;
}

int Kernel<float>::predict_device(int m, const float* dtest, float* dpred) const {
  if (!fitted() || m < 0) return 1;
  if (m == 0) return 0;
  if (!hssk_is_device_pointer(dtest) || !hssk_is_device_pointer(dpred)) return 2;
  run_predict(m, nullptr, 0, dtest, nullptr, nullptr, dpred);
  return 0;
}

}  // namespace kernel
}  // namespace strumpack
