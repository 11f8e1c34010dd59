// Private to Kernel.cpp, KernelGradient.cpp, KernelKrylov.cpp, KernelFloat.cpp and KernelC.cpp: the kept model of Kernel<double>, the
// device blocks of its Krylov calls and the small helpers those files share.  Kernel.hpp and everything a user compiles against
// stay free of it.
#pragma once
#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "DevicePool.hpp"
#include "HSSMatrix.hpp"
#include "Kernel.hpp"
#include "hssk.h"

namespace strumpack {
namespace kernel {

inline void ckk(int rc) { if (rc) throw std::runtime_error(hssk_last_error()); }

// f() between the start and the stop of stopwatch id.  A plain call after f(), not a destructor: when f() throws the stopwatch
// stays open, which hssk_watch_start and hssk_watch_read_ms handle, and no event is recorded on a stream that may just have failed.
template <class F> inline void watched(hssk_ctx* ctx, int id, F&& f) { hssk_watch_start(ctx, id); f(); hssk_watch_stop(ctx, id); }

// the products with the exact kernel matrix (hssk_kernel_matmul and its kin) exist for Gauss and Laplace kernels only
inline bool exact_products(const Kernel<double>& K) { return K.device_type() == 0 || K.device_type() == 1; }
inline void require_exact_products(const Kernel<double>& K, const char* what) {
  if (!exact_products(K)) throw std::invalid_argument(std::string(what) + ": Gauss and Laplace kernels only");
}

// the kernel of K over the kept, cluster-ordered points dX of its model, with `diagonal` (0 or lambda) on the diagonal
inline hssk_kernel_spec kept_spec(const Kernel<double>& K, const double* dX, double diagonal) {
  return hssk_kernel_spec{dX, (long long)K.n(), int(K.d()), K.device_type(), K.degree(), K.width(), diagonal};
}

// the built-in kernel of device type `type` (0 Gauss, 1 Laplace, 2 ANOVA of degree p); null for any other type
template <typename T> std::unique_ptr<Kernel<T>> make_kernel(int type, DenseMatrix<T>& data, T h, T lambda, int p) {
  switch (type) {
    case 0: return std::unique_ptr<Kernel<T>>(new GaussKernel<T>(data, h, lambda));
    case 1: return std::unique_ptr<Kernel<T>>(new LaplaceKernel<T>(data, h, lambda));
    case 2: return std::unique_ptr<Kernel<T>>(new ANOVAKernel<T>(data, h, lambda, p));
    default: return nullptr;
  }
}

// of the last fit_HSS of this thread: what SPX_kernel_fit_info and SPX_kernel_node_info hand out (Kernel.cpp)
const long long* last_fit_info();
const std::vector<int>& last_fit_nodes();

// ---- the kept model of Kernel<double> ------------------------------------------------------------------------------------------
struct Kernel<double>::Model {
  HSS::HSSMatrix<double> H;            // compressed K + lambda I with its ULV factors
  std::vector<double> labels;          // in cluster order
  DenseMatrix<double> weights;
  double* dX = nullptr;                // cluster-ordered points, d x n (device pool)
  size_t bX = 0;
  explicit Model(HSS::HSSMatrix<double>&& h) : H(std::move(h)) {}
  hssk_ctx* ctx() const { return H.engine()->ctx(); }
  ~Model() {
    if (dX) {
      hssk_sync(ctx());   // (nothing in flight may still read the chunk)
      DevicePool::get().release(dX, bX);
    }
  }
};

// the device blocks of a Krylov call, for blocks of at most ncmax columns: restart + 1 basis blocks, Z (what the ULV solve works
// on: always this buffer, so that its recorded sweep is replayed), W (the product; the residual's A x at the start of a cycle),
// U (the update), B and X for callers that have none, and the small coefficient arrays
struct Kernel<double>::KrylovWork {
  long long n;
  int ncmax, m;   // m: steps of a cycle = min(restart, maxit)
  PoolBuf bV, bZ, bW, bU, bB, bX, bS, bP;
  double *V, *Z, *W, *U, *B, *X, *Y, *Hout, *norms, *ones;
  void* prep = nullptr;   // mixed mode: the prepared float points of hssk_kernel_matmul_f32 (prep_bytes > 0)
  std::size_t prep_bytes;
  KrylovWork(hssk_ctx* ctx, long long n_, int ncmax_, int maxit, int restart, bool own_bx, std::size_t prep_bytes_ = 0)
      : n(n_), ncmax(ncmax_), m(std::min(restart, maxit)), bV(ctx, sizeof(double) * n_ * ncmax_ * (size_t)(m + 1)), bZ(ctx, sizeof(double) * n_ * ncmax_),
        bW(ctx, sizeof(double) * n_ * ncmax_), bU(ctx, sizeof(double) * n_ * ncmax_), bB(ctx, sizeof(double) * n_ * ncmax_),
        bX(ctx, own_bx ? sizeof(double) * n_ * ncmax_ : 0), bS(ctx, sizeof(double) * (size_t)ncmax_ * (2 * m + 4)), bP(ctx, prep_bytes_),
        prep_bytes(prep_bytes_) {
    if (prep_bytes) prep = bP.p;
    V = (double*)bV.p; Z = (double*)bZ.p; W = (double*)bW.p; U = (double*)bU.p; B = (double*)bB.p; X = (double*)bX.p;
    Y = (double*)bS.p; Hout = Y + (size_t)ncmax * m; norms = Hout + (size_t)ncmax * (m + 2); ones = norms + ncmax;
    const std::vector<double> one(ncmax, 1.);
    ckk(hssk_memcpy_h2d(ctx, ones, one.data(), (long long)sizeof(double) * ncmax));
  }
};

}  // namespace kernel
}  // namespace strumpack
