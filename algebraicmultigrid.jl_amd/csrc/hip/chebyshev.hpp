// chebyshev.hpp — the host half of the Chebyshev polynomial smoother and the spectral-radius estimate it takes its default
// bounds from.  Included by amghip.hip (after csr_ops.hpp).
//
// The iteration, for the smoother matrix S, D = diag(S), bounds 0 < lo < hi on the eigenvalues of D^-1 S and degree >= 1:
//   theta = (hi + lo) / 2, delta = (hi - lo) / 2, sigma = theta / delta, rho = 1 / sigma
//   d = (1 / theta) D^-1 (b - S x);  x += d
//   k = 2 .. degree:  rho' = 1 / (2 sigma - rho);  d = (rho' rho) d + (2 rho' / delta) D^-1 (b - S x);  x += d;  rho = rho'
// — the three-term recurrence of the scaled Chebyshev polynomials (Saad, Iterative Methods for Sparse Linear Systems, alg. 12.1;
// PyAMG's polynomial smoother, hypre's and AmgX's Chebyshev relaxations use the same).  Step k is one pass of csr_stream_kernel in
// mode M_CHEB1 / M_CHEB with the pair (c1, c2)_k computed here, on the host, in double.
#pragma once
#include <cmath>
#include <vector>

namespace {

constexpr int kChebMaxDegree = 16;      // a polynomial smoother of higher degree is a solver, not a smoother: refused
constexpr int kLanczosSteps = 15;       // default length of the Lanczos process of the estimate
constexpr double kChebLower = 1.0 / 30.0, kChebUpper = 1.1;   // default bounds as factors of the estimate (PyAMG's)

inline bool cheb_bounds_valid(double lo, double hi) { return std::isfinite(lo) && std::isfinite(hi) && lo > 0.0 && lo < hi; }

// c[2 k] = c1, c[2 k + 1] = c2 of step k + 1 (c1 of the first step is 0 and is never applied)
inline void cheb_coefficients(int degree, double lo, double hi, double* c) {
  const double theta = (hi + lo) / 2.0, delta = (hi - lo) / 2.0, sigma = theta / delta;
  double rho = 1.0 / sigma;
  c[0] = 0.0;
  c[1] = 1.0 / theta;
  for (int k = 1; k < degree; ++k) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    c[2 * k] = rho_new * rho;
    c[2 * k + 1] = 2.0 * rho_new / delta;
    rho = rho_new;
  }
}

// one side (pre / post) of a level: the bounds as the caller gave them — eigenvalue bounds, or factors of the estimate made at
// amgh_finalize — and the coefficients once they are known
struct ChebSide {
  double lo = kChebLower, hi = kChebUpper;
  bool relative = true;
  std::vector<double> c;   // 2 x degree, empty until the bounds are absolute
};

// eigenvalues of the symmetric tridiagonal matrix (diagonal a[0..m), off-diagonal b[0..m-1)) below x: a Sturm count
inline int tridiag_count_below(const std::vector<double>& a, const std::vector<double>& b, int m, double x) {
  int cnt = 0;
  double q = 1.0;
  for (int i = 0; i < m; ++i) {
    const double off = i > 0 ? b[(size_t)i - 1] * b[(size_t)i - 1] : 0.0;
    q = a[(size_t)i] - x - (i > 0 ? off / q : 0.0);
    if (q == 0.0) q = -1e-300;
    if (q < 0.0) ++cnt;
  }
  return cnt;
}
// its eigenvalue of largest magnitude, by bisection between the Gershgorin bounds
inline double tridiag_spectral_radius(const std::vector<double>& a, const std::vector<double>& b, int m) {
  double gl = a[0], gu = a[0];
  for (int i = 0; i < m; ++i) {
    const double r = (i > 0 ? std::fabs(b[(size_t)i - 1]) : 0.0) + (i + 1 < m ? std::fabs(b[(size_t)i]) : 0.0);
    gl = std::min(gl, a[(size_t)i] - r);
    gu = std::max(gu, a[(size_t)i] + r);
  }
  auto kth = [&](int k) {   // the k-th smallest eigenvalue (0-based)
    double lo = gl, hi = gu;
    for (int it = 0; it < 200 && hi - lo > 4e-16 * std::max(std::fabs(lo), std::fabs(hi)); ++it) {
      const double mid = 0.5 * (lo + hi);
      if (tridiag_count_below(a, b, m, mid) > k) hi = mid; else lo = mid;
    }
    return 0.5 * (lo + hi);
  };
  return std::max(std::fabs(kth(0)), std::fabs(kth(m - 1)));
}

// ---- Lanczos for D^-1 S in the D-inner product <u, v> = sum d_i u_i v_i (S symmetric: D^-1 S is self-adjoint in it) -----------
// start vector: U[0, 1) of the splitmix64 stream the benchmarks and tests draw from (state_i = seed + (i + 1) 0x9E3779B97F4A7C15)
__global__ void lz_init_kernel(real* v, int64_t n, unsigned long long seed) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long z = seed + (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    v[i] = (real)((double)(z >> 11) * (1.0 / 9007199254740992.0));
  }
}
// w = D^-1 w where it is given (rows without a diagonal: 0); partial[b] = this block's share of sum d w v (v = nullptr: sum d w w)
__global__ __launch_bounds__(kThreads) void lz_scale_dot_kernel(real* w, const real* v, const real* diag, int64_t n, int scale, real* partial) {
  __shared__ real s_part[kThreads / kWave];
  real acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const real dg = diag[i];
    real wi = w[i];
    if (scale) { wi = (dg == 0.0) ? (real)0.0 : wi / dg; w[i] = wi; }
    acc += dg * wi * (v ? v[i] : wi);
  }
  const real r = block_reduce_sum(acc, s_part);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
// w = w - alpha v - beta u; partial: sum d w w
__global__ __launch_bounds__(kThreads) void lz_update_kernel(real* w, const real* v, const real* u, const real* diag, int64_t n, real alpha, real beta,
                                                               real* partial) {
  __shared__ real s_part[kThreads / kWave];
  real acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const real wi = (w[i] - alpha * v[i]) - beta * u[i];
    w[i] = wi;
    acc += diag[i] * wi * wi;
  }
  const real r = block_reduce_sum(acc, s_part);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
// u = v; v = w * s
__global__ void lz_shift_kernel(real* u, real* v, const real* w, int64_t n, real s) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    u[i] = v[i];
    v[i] = w[i] * s;
  }
}

// *out = the largest |Ritz value| of `steps` Lanczos steps (clamped to n) for D^-1 M, M square and symmetric with a positive
// diagonal (not checked: for another M the number is whatever the recurrence gives).  Allocates 3 n + 1024 reals for the call,
// synchronises st after every step (two sums come back to the host: setup-time work).  AMGH_EINVAL when the result is not a
// positive finite number (e.g. an all-zero diagonal).
int csr_spectral_radius(amgh_csr* M, int steps, unsigned long long seed, hipStream_t st, double* out) {
  if (!M || !out || M->nrows != M->ncols || M->nrows <= 0 || steps < 1) return AMGH_EINVAL;
  const int64_t n = M->nrows;
  const int m = (int)std::min<int64_t>(steps, n);
  RC_TRY(csr_ensure_diag(M, st));
  real *u = nullptr, *v = nullptr, *w = nullptr, *part = nullptr;
  int rc = dev_alloc(&u, n);
  if (rc == AMGH_OK) rc = dev_alloc(&v, n);
  if (rc == AMGH_OK) rc = dev_alloc(&w, n);
  if (rc == AMGH_OK) rc = dev_alloc(&part, kRedBlocks);
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(kRedBlocks, (n + kThreads - 1) / kThreads));
  std::vector<real> hp((size_t)nb);
  auto sum_back = [&](double* s) -> int {   // the partial sums, added on the host in block order
    if (hipMemcpyAsync(hp.data(), part, sizeof(real) * (size_t)nb, hipMemcpyDeviceToHost, st) != hipSuccess) return -1001;
    if (hipStreamSynchronize(st) != hipSuccess) return -1001;
    double t = 0.0;
    for (int i = 0; i < nb; ++i) t += (double)hp[(size_t)i];
    *s = t;
    return AMGH_OK;
  };
  std::vector<double> al, be;
  double nrm2 = 0.0;
  if (rc == AMGH_OK && hipMemsetAsync(u, 0, sizeof(real) * n, st) != hipSuccess) rc = -1001;
  if (rc == AMGH_OK) {
    hipLaunchKernelGGL(lz_init_kernel, dim3(grid_for(n)), dim3(256), 0, st, w, n, seed);
    hipLaunchKernelGGL(lz_scale_dot_kernel, dim3(nb), dim3(kThreads), 0, st, w, (const real*)nullptr, (const real*)M->diag, n, 0, part);
    rc = sum_back(&nrm2);
  }
  if (rc == AMGH_OK && !(nrm2 > 0.0 && std::isfinite(nrm2))) rc = AMGH_EINVAL;
  if (rc == AMGH_OK) hipLaunchKernelGGL(lz_shift_kernel, dim3(grid_for(n)), dim3(256), 0, st, u, v, (const real*)w, n, (real)(1.0 / std::sqrt(nrm2)));
  if (rc == AMGH_OK && hipMemsetAsync(u, 0, sizeof(real) * n, st) != hipSuccess) rc = -1001;
  double beta = 0.0;
  for (int j = 0; j < m && rc == AMGH_OK; ++j) {
    rc = csr_apply(M, M_SPMV, v, nullptr, w, st);
    if (rc != AMGH_OK) break;
    double alpha = 0.0, b2 = 0.0;
    hipLaunchKernelGGL(lz_scale_dot_kernel, dim3(nb), dim3(kThreads), 0, st, w, (const real*)v, (const real*)M->diag, n, 1, part);
    rc = sum_back(&alpha);
    if (rc != AMGH_OK) break;
    hipLaunchKernelGGL(lz_update_kernel, dim3(nb), dim3(kThreads), 0, st, w, (const real*)v, (const real*)u, (const real*)M->diag, n, (real)alpha,
                       (real)beta, part);
    rc = sum_back(&b2);
    if (rc != AMGH_OK) break;
    al.push_back(alpha);
    if (!std::isfinite(alpha) || !std::isfinite(b2)) { rc = AMGH_EINVAL; break; }
    beta = std::sqrt(std::max(b2, 0.0));
    if (j + 1 == m || !(beta > 1e-13 * std::fabs(alpha))) break;   // an invariant subspace: the Ritz values are eigenvalues
    be.push_back(beta);
    hipLaunchKernelGGL(lz_shift_kernel, dim3(grid_for(n)), dim3(256), 0, st, u, v, (const real*)w, n, (real)(1.0 / beta));
  }
  if (rc == AMGH_OK && hipGetLastError() != hipSuccess) rc = -1001;
  hipFree(u); hipFree(v); hipFree(w); hipFree(part);
  RC_TRY(rc);
  if (al.empty()) return AMGH_EINVAL;
  const double rho = tridiag_spectral_radius(al, be, (int)al.size());
  if (!(rho > 0.0) || !std::isfinite(rho)) return AMGH_EINVAL;
  *out = rho;
  return AMGH_OK;
}

}  // namespace
