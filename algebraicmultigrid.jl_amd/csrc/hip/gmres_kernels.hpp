// gmres_kernels.hpp — gfx950 kernels of the device-resident restarted GMRES (amgh_gmres, amghip.hip: gmres_dev).
//
// The Krylov basis V is (restart + 1) columns of n reals, each column starting on a 256-byte boundary (leading
// dimension ld).  The orthogonalisation of w = V[:, k] against V[:, 0:k] is classical Gram-Schmidt with the DGKS
// re-orthogonalisation test, as IterativeSolvers.jl's gmres does it, in a FIXED launch plan per Arnoldi step:
//   pass p = 0, 1, 2:  gmres_dots_kernel    partial[b][j] = sum_i V[i, j] w[i], j < k         (one pass over the k columns)
//                      gmres_reduce_kernel  coef = sum_b partial[b], H[:, k-1] (+)= coef, proj = |coef|
//                      gmres_update_kernel  w -= V coef, partial[b] = sum_i w[i]^2            (w read once, written once)
//                      gmres_norm_kernel    nrm = |w|; nrm < proj / sqrt(2) and p < 2: another pass is pending;
//                                           otherwise H[k, k-1] = nrm, the null-vector residual estimate, 1 / nrm
//   passes 1 and 2 are the same launches reading the pending flag and returning when it is clear: the DGKS decision
//   never travels to the host.  The repetition is capped at kGmMaxExtra = 2 extra passes.
// Every reduction is per-block partials summed by one workgroup in a fixed order (no atomics): a run is bitwise
// reproducible.  The tall-skinny products stream V with 16-byte loads; a thread keeps its rows of w in registers and
// one accumulator per column (KC = 8 / 16 / 32 / 64 columns, the smallest that holds k).
#pragma once
#include "amghip_kernels.hpp"

namespace amgh {

constexpr int kGmMaxRestart = 64;
constexpr int kGmMaxExtra = 2;                           // DGKS re-orthogonalisation passes per step, at most
constexpr int kGmLdH = kGmMaxRestart + 1;                // H is (restart + 1) x restart, column-major, leading dimension 65
// the device scalar block (reals)
constexpr int kGmH = 0;                                  // H[i + kGmLdH * j]
constexpr int kGmNull = kGmLdH * kGmMaxRestart;          // null vector of H[1:k+1, 1:k]' (the residual estimate), 65
constexpr int kGmCoef = kGmNull + kGmLdH;                // projection coefficients of the current pass, 64
constexpr int kGmY = kGmCoef + kGmMaxRestart;            // least-squares solution, 64
constexpr int kGmS = kGmY + kGmMaxRestart;               // [0] current  [1] beta  [2] acc  [3] proj  [4] nrm  [5] scale
constexpr int kGmReals = kGmS + 8;
// device ints: [0] a re-orthogonalisation pass is pending, [1] extra passes run since the handle's counter was cleared
constexpr int kGmFlags = 2;

constexpr int kGmVW = 16 / (int)sizeof(real);            // reals per 16-byte load
typedef real gm_vec_t __attribute__((ext_vector_type(kGmVW)));

__device__ __forceinline__ real gm_wave_sum(real v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;  // valid on lane 0
}

// partial[b * kGmMaxRestart + j] = sum over this block's rows of V[i, j] * w[i], j < k.  Rows in 16-byte vectors, grid-stride;
// the n % kGmVW tail rows belong to thread 0 of block 0.
template <int KC>
__global__ __launch_bounds__(kThreads) void gmres_dots_kernel(const real* __restrict__ V, int64_t ld, int k, const real* __restrict__ w,
                                                              int64_t n, real* __restrict__ partial, const int* flags, int pass) {
  if (pass > 0 && flags[0] == 0) return;
  __shared__ real s_red[kThreads / kWave][KC];
  real acc[KC];
#pragma unroll
  for (int j = 0; j < KC; ++j) acc[j] = 0.0;
  const int64_t nv = n / kGmVW;
  const gm_vec_t* wv = reinterpret_cast<const gm_vec_t*>(w);
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nv; p += (int64_t)gridDim.x * blockDim.x) {
    const gm_vec_t wi = wv[p];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      if (j < k) {
        const gm_vec_t vj = reinterpret_cast<const gm_vec_t*>(V + j * ld)[p];
        real s = vj[0] * wi[0];
#pragma unroll
        for (int e = 1; e < kGmVW; ++e) s += vj[e] * wi[e];
        acc[j] += s;
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t i = nv * kGmVW; i < n; ++i) {
      const real wi = w[i];
#pragma unroll
      for (int j = 0; j < KC; ++j)
        if (j < k) acc[j] += V[j * ld + i] * wi;
    }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    if (j < k) {
      const real t = gm_wave_sum(acc[j]);
      if (lane == 0) s_red[wave][j] = t;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < k) {
    real t = s_red[0][threadIdx.x];
    for (int q = 1; q < kThreads / kWave; ++q) t += s_red[q][threadIdx.x];
    partial[blockIdx.x * (int64_t)kGmMaxRestart + threadIdx.x] = t;
  }
}

// One workgroup: coef[j] = sum_b partial[b][j] (four fixed quarters of the blocks, added in order), H[j, col] = coef[j] on
// pass 0 and += coef[j] on the re-orthogonalisation passes, proj = |coef|.
__global__ __launch_bounds__(kThreads) void gmres_reduce_kernel(const real* __restrict__ partial, int nb, int k, int col, real* sc,
                                                                const int* flags, int pass) {
  if (pass > 0 && flags[0] == 0) return;
  constexpr int Q = kThreads / kGmMaxRestart;
  __shared__ real s_q[Q][kGmMaxRestart];
  __shared__ real s_c[kGmMaxRestart];
  const int j = threadIdx.x % kGmMaxRestart, q = threadIdx.x / kGmMaxRestart;
  const int per = (nb + Q - 1) / Q, b0 = q * per, b1 = min(nb, b0 + per);
  if (j < k) {
    real v = 0.0;
    for (int b = b0; b < b1; ++b) v += partial[b * (int64_t)kGmMaxRestart + j];
    s_q[q][j] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < k) {
    real c = s_q[0][threadIdx.x];
    for (int t = 1; t < Q; ++t) c += s_q[t][threadIdx.x];
    s_c[threadIdx.x] = c;
    sc[kGmCoef + threadIdx.x] = c;
    real* H = sc + kGmH + (int64_t)kGmLdH * col;
    H[threadIdx.x] = pass > 0 ? H[threadIdx.x] + c : c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    real p = 0.0;
    for (int t = 0; t < k; ++t) p += s_c[t] * s_c[t];
    sc[kGmS + 3] = sqrt(p);
  }
}

// w -= V[:, 0:k] coef, and partial[b] = sum over this block's rows of the new w[i]^2.
template <int KC>
__global__ __launch_bounds__(kThreads) void gmres_update_kernel(const real* __restrict__ V, int64_t ld, int k, real* __restrict__ w,
                                                                int64_t n, const real* __restrict__ sc, real* __restrict__ partial,
                                                                const int* flags, int pass) {
  if (pass > 0 && flags[0] == 0) return;
  __shared__ real s_part[kThreads / kWave];
  real c[KC];
#pragma unroll
  for (int j = 0; j < KC; ++j) c[j] = j < k ? sc[kGmCoef + j] : 0.0;
  real acc = 0.0;
  const int64_t nv = n / kGmVW;
  gm_vec_t* wv = reinterpret_cast<gm_vec_t*>(w);
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nv; p += (int64_t)gridDim.x * blockDim.x) {
    gm_vec_t s = reinterpret_cast<const gm_vec_t*>(V)[p] * c[0];
#pragma unroll
    for (int j = 1; j < KC; ++j)
      if (j < k) s += reinterpret_cast<const gm_vec_t*>(V + j * ld)[p] * c[j];
    const gm_vec_t wi = wv[p] - s;
    wv[p] = wi;
#pragma unroll
    for (int e = 0; e < kGmVW; ++e) acc += wi[e] * wi[e];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t i = nv * kGmVW; i < n; ++i) {
      real s = V[i] * c[0];
#pragma unroll
      for (int j = 1; j < KC; ++j)
        if (j < k) s += V[j * ld + i] * c[j];
      const real wi = w[i] - s;
      w[i] = wi;
      acc += wi * wi;
    }
  const real t = block_reduce_sum(acc, s_part);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// One workgroup: nrm = sqrt(sum_b partial[b]) and the DGKS decision for column col of H.  Another pass is pending when
// nrm < proj / sqrt(2) and fewer than kGmMaxExtra extra passes have run; otherwise the step is complete:
//   H[col+1, col] = nrm, and IterativeSolvers' residual estimate
//   nullvec[col+1] = -dot(nullvec[0:col+1], H[0:col+1, col]) / nrm ; acc += nullvec[col+1]^2 ; current = beta / sqrt(acc)
// Lucky breakdown (nrm == 0): current = 0 and the scale is 0 (the column is never used).
__global__ __launch_bounds__(kThreads) void gmres_norm_kernel(const real* __restrict__ partial, int nb, int col, real* sc, int* flags,
                                                              int pass) {
  if (pass > 0 && flags[0] == 0) return;
  __shared__ real s_part[kThreads / kWave];
  real v = 0.0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) v += partial[i];
  const real r = block_reduce_sum(v, s_part);
  if (threadIdx.x != 0) return;
  const real nrm = sqrt(r);
  if (pass < kGmMaxExtra && nrm < sc[kGmS + 3] / sqrt((real)2.0)) {
    flags[0] = 1;
    flags[1] += 1;
    return;
  }
  flags[0] = 0;
  real* H = sc + kGmH + (int64_t)kGmLdH * col;
  H[col + 1] = nrm;
  sc[kGmS + 4] = nrm;
  if (nrm == 0.0) {
    sc[kGmS + 0] = 0.0;
    sc[kGmS + 5] = 0.0;
    return;
  }
  real* nv = sc + kGmNull;
  real d = 0.0;
  for (int i = 0; i <= col; ++i) d += nv[i] * H[i];
  const real nu = -d / nrm;
  nv[col + 1] = nu;
  const real acc = sc[kGmS + 2] + nu * nu;
  sc[kGmS + 2] = acc;
  sc[kGmS + 0] = sc[kGmS + 1] / sqrt(acc);
  sc[kGmS + 5] = 1.0 / nrm;
}

// (Re)start, after sc[kGmS + 1] = beta = |v1|: nullvec = e1, acc = 1, current = beta, scale = 1 / beta (0 when beta == 0).
__global__ void gmres_start_kernel(real* sc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const real beta = sc[kGmS + 1];
  sc[kGmNull] = 1.0;
  sc[kGmS + 2] = 1.0;
  sc[kGmS + 0] = beta;
  sc[kGmS + 5] = beta != 0.0 ? 1.0 / beta : 0.0;
}

// v *= scale[0]
__global__ __launch_bounds__(256) void gmres_scale_kernel(real* v, const real* scale, int64_t n) {
  const real s = scale[0];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = v[i] * s;
}

// One workgroup: min_y |beta e1 - H[0:k+1, 0:k] y| by Givens rotations (IterativeSolvers' FastHessenberg ldiv!) and back
// substitution, k <= kGmMaxRestart.  Rotation i: r = sqrt(a^2 + b^2), c = a / r, s = b / r (c = 1, s = 0 when r == 0), applied
// to rows i, i+1 of the columns right of i (one thread per column) and of the right-hand side.
__global__ __launch_bounds__(kThreads) void gmres_lsq_kernel(real* sc, int k) {
  __shared__ real sH[kGmLdH * kGmMaxRestart];
  __shared__ real rhs[kGmLdH];
  __shared__ real s_cs[2];
  for (int t = threadIdx.x; t < kGmLdH * k; t += blockDim.x) sH[t] = sc[kGmH + t];
  for (int t = threadIdx.x; t <= k; t += blockDim.x) rhs[t] = t == 0 ? sc[kGmS + 1] : 0.0;
  __syncthreads();
  for (int i = 0; i < k; ++i) {
    if (threadIdx.x == 0) {
      const real a = sH[i + kGmLdH * i], b = sH[i + 1 + kGmLdH * i];
      const real r = sqrt(a * a + b * b);
      const real c = r != 0.0 ? a / r : 1.0, s = r != 0.0 ? b / r : 0.0;
      sH[i + kGmLdH * i] = c * a + s * b;
      sH[i + 1 + kGmLdH * i] = 0.0;
      const real t = -s * rhs[i] + c * rhs[i + 1];
      rhs[i] = c * rhs[i] + s * rhs[i + 1];
      rhs[i + 1] = t;
      s_cs[0] = c; s_cs[1] = s;
    }
    __syncthreads();
    const real c = s_cs[0], s = s_cs[1];
    for (int j = i + 1 + threadIdx.x; j < k; j += blockDim.x) {
      const real hi = sH[i + kGmLdH * j], hn = sH[i + 1 + kGmLdH * j];
      sH[i + kGmLdH * j] = c * hi + s * hn;
      sH[i + 1 + kGmLdH * j] = -s * hi + c * hn;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    real* y = sc + kGmY;
    for (int i = k - 1; i >= 0; --i) {
      real t = rhs[i];
      for (int j = i + 1; j < k; ++j) t -= sH[i + kGmLdH * j] * y[j];
      y[i] = t / sH[i + kGmLdH * i];
    }
  }
}

// x += V[:, 0:k] y (the sum over the columns in order, then added to x)
__global__ __launch_bounds__(256) void gmres_xupdate_kernel(const real* __restrict__ V, int64_t ld, int k, const real* __restrict__ sc,
                                                            real* __restrict__ x, int64_t n) {
  __shared__ real s_y[kGmMaxRestart];
  if ((int)threadIdx.x < k) s_y[threadIdx.x] = sc[kGmY + threadIdx.x];
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    real s = V[i] * s_y[0];
    for (int j = 1; j < k; ++j) s += V[j * ld + i] * s_y[j];
    x[i] = x[i] + s;
  }
}

}  // namespace amgh
