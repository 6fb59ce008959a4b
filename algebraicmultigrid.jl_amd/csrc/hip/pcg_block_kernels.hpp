// pcg_block_kernels.hpp — gfx950 kernels of the device-resident PCG on a block of right-hand sides (amgh_pcg_block,
// amghip.hip: pcg_block_dev).
//
// nrhs independent cg's: column j runs IterativeSolvers.jl's recurrence (the one pcg_dev restates) on its own right-hand
// side; the columns share no Krylov space.  r, c, u and x are n x nrhs, column-major, columns n apart.  An iteration is a
// FIXED launch plan whatever the number of active columns (the cycle and the SpMV run every column of the block):
//   cycle / copy         c = Pl \ r                                             (apply_cycle on the block)
//   pcg_block_dots       partial[j][b] = sum over block b's rows of c_j r_j       (active columns)
//   pcg_block_scal 0     rho_prev = rho, rho = sum_b partial, beta = rho / rho_prev
//   pcg_block_xpby       u_j = c_j + beta_j u_j                                   (active columns)
//   csr_apply(ncolv)     c = A u                                                  (every column)
//   pcg_block_dots       partial[j][b] = sum over block b's rows of u_j c_j       (active columns)
//   pcg_block_scal 1     u.c = sum_b partial, alpha = rho / u.c
//   pcg_block_update     x_j += alpha_j u_j, r_j -= alpha_j c_j, partial = |r_j|^2 first stage (active columns); c = 0
//   pcg_block_scal 2     |r_j| = sqrt(sum_b partial), iters_j += 1, the column freezes when !(|r_j| > tol_j) or
//                        iters_j == maxiter; the active count: the status record the host reads in one copy
// A column's predicate is the device flag PbStatus::active[j], read by every kernel; the host never decides it.  Frozen
// columns keep r_j as it was (not zeroed): the cycle and the SpMV map every column on its own, so whatever a frozen column
// holds never reaches another column's bits.
// Every reduction is per-block partials over a row partition that depends on n only, summed by one workgroup in a fixed
// order (no atomics): a run is bitwise reproducible, and a column's bits do not depend on the other columns' values.
// Rows travel in 16-byte vectors when n is a multiple of the vector width (then every column of the workspace starts on a
// 16-byte boundary), one real at a time otherwise.
#pragma once
#include "amghip_kernels.hpp"

namespace amgh {

constexpr int kPbMaxCols = 64;
constexpr int kPbScalThreads = 1024;                      // the scalar step: a group of kPbScalThreads / pow2(nrhs) lanes per column
// the device scalar block: sc[q * kPbMaxCols + j]
constexpr int kPbRho = 0, kPbRhoPrev = 1, kPbBeta = 2, kPbAlpha = 3, kPbUc = 4, kPbTol = 5;
constexpr int kPbScal = 6;
// per-column state and the record the host copies once per iteration
struct PbStatus {
  real res[kPbMaxCols];     // |r_j| after iters[j] iterations
  int iters[kPbMaxCols];
  int active[kPbMaxCols];   // 1: the column iterates on
  int nactive;
  int pad[3];
};

template <int W>
struct alignas(W * sizeof(real)) PbVec {
  real v[W];
};

__device__ __forceinline__ real pb_wave_sum(real v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;  // valid on lane 0
}

// partial[j * kRedBlocks + blockIdx.x] = sum over this block's rows of a_j[i] * b_j[i], for the active columns (all: every
// column).  Rows in W-wide vectors, grid-stride; the sum of a vector's W products is formed first, then accumulated.
template <int W>
__global__ __launch_bounds__(kThreads) void pcg_block_dots_kernel(const real* __restrict__ a, const real* __restrict__ b, int64_t n,
                                                                  int bs, const PbStatus* __restrict__ st, int all,
                                                                  real* __restrict__ partial) {
  __shared__ real s_red[kThreads / kWave][kPbMaxCols];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t nv = n / W;
  for (int j = 0; j < bs; ++j) {
    if (!all && !st->active[j]) continue;   // (uniform over the grid)
    const PbVec<W>* av = reinterpret_cast<const PbVec<W>*>(a + j * n);
    const PbVec<W>* bv = reinterpret_cast<const PbVec<W>*>(b + j * n);
    real acc = 0.0;
#pragma unroll 4
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nv; p += (int64_t)gridDim.x * blockDim.x) {
      const PbVec<W> x = av[p], y = bv[p];
      real s = x.v[0] * y.v[0];
#pragma unroll
      for (int e = 1; e < W; ++e) s += x.v[e] * y.v[e];
      acc += s;
    }
    const real t = pb_wave_sum(acc);
    if (lane == 0) s_red[wave][j] = t;
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < bs && (all || st->active[j])) {
    real t = s_red[0][j];
    for (int q = 1; q < kThreads / kWave; ++q) t += s_red[q][j];
    partial[(int64_t)j * kRedBlocks + blockIdx.x] = t;
  }
}

// One workgroup of kPbScalThreads: column j's G = kPbScalThreads / P lanes (P = the power of two >= bs) sum its nb partials
// (lane g takes b = g, g + G, ...), then a tree over the G lanes in LDS; lane 0 of the group runs the scalar step:
//   which 3 (start):  |r_j| = sqrt(sum), tol_j = max(reltol |r_j|, abstol), rho_j = 1, iters_j = 0, active_j = maxiter > 0 && |r_j| > tol_j
//   which 0:          rho_prev = rho, rho = sum, beta = rho / rho_prev
//   which 1:          u.c = sum, alpha = rho / u.c
//   which 2:          |r_j| = sqrt(sum), iters_j += 1, active_j = iters_j < maxiter && |r_j| > tol_j
// on the active columns; which 2 and 3 also count the active columns into the status record.
__global__ __launch_bounds__(kPbScalThreads) void pcg_block_scal_kernel(const real* __restrict__ partial, int nb, int bs, real* sc,
                                                                        PbStatus* st, int which, int maxiter, double abstol,
                                                                        double reltol) {
  __shared__ real s_v[kPbScalThreads];
  __shared__ int s_act[kPbMaxCols];
  int P = 1;
  while (P < bs) P <<= 1;
  const int G = kPbScalThreads / P;
  const int j = threadIdx.x / G, g = threadIdx.x % G;
  const bool live = j < bs && (which == 3 || st->active[j]);
  real v = 0.0;
  if (live)
    for (int b = g; b < nb; b += G) v += partial[(int64_t)j * kRedBlocks + b];
  s_v[threadIdx.x] = v;
  __syncthreads();
  for (int s = G / 2; s > 0; s >>= 1) {
    if (g < s) s_v[threadIdx.x] += s_v[threadIdx.x + s];
    __syncthreads();
  }
  if (g == 0 && j < bs) {
    const real r = s_v[threadIdx.x];
    real* col = sc + j;
    if (which == 3) {
      const real res = sqrt(r);
      const double t = reltol * (double)res;
      const real tol = (real)(t < abstol ? abstol : t);   // std::max(reltol * |r0|, abstol), as pcg_dev
      col[kPbTol * kPbMaxCols] = tol;
      col[kPbRho * kPbMaxCols] = 1.0;
      st->res[j] = res;
      st->iters[j] = 0;
      st->active[j] = (0 < maxiter && res > tol) ? 1 : 0;
    } else if (live) {
      if (which == 0) {
        const real rp = col[kPbRho * kPbMaxCols];
        col[kPbRhoPrev * kPbMaxCols] = rp;
        col[kPbRho * kPbMaxCols] = r;
        col[kPbBeta * kPbMaxCols] = r / rp;
      } else if (which == 1) {
        col[kPbUc * kPbMaxCols] = r;
        col[kPbAlpha * kPbMaxCols] = col[kPbRho * kPbMaxCols] / r;
      } else {
        const real res = sqrt(r);
        const int it = st->iters[j] + 1;
        st->res[j] = res;
        st->iters[j] = it;
        st->active[j] = (it < maxiter && res > col[kPbTol * kPbMaxCols]) ? 1 : 0;
      }
    }
    if (which >= 2) s_act[j] = st->active[j];
  }
  if (which < 2) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int q = 0; q < bs; ++q) c += s_act[q];
    st->nactive = c;
  }
}

// u_j = c_j + beta_j u_j on the active columns
template <int W>
__global__ __launch_bounds__(kThreads) void pcg_block_xpby_kernel(real* __restrict__ u, const real* __restrict__ c, int64_t n, int bs,
                                                                  const real* __restrict__ sc, const PbStatus* __restrict__ st) {
  const int64_t nv = n / W;
  for (int j = 0; j < bs; ++j) {
    if (!st->active[j]) continue;
    const real be = sc[kPbBeta * kPbMaxCols + j];
    PbVec<W>* uv = reinterpret_cast<PbVec<W>*>(u + j * n);
    const PbVec<W>* cv = reinterpret_cast<const PbVec<W>*>(c + j * n);
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nv; p += (int64_t)gridDim.x * blockDim.x) {
      PbVec<W> w = uv[p];
      const PbVec<W> ci = cv[p];
#pragma unroll
      for (int e = 0; e < W; ++e) w.v[e] = ci.v[e] + be * w.v[e];
      uv[p] = w;
    }
  }
}

// Active columns: x_j += alpha_j u_j, r_j -= alpha_j c_j, partial[j * kRedBlocks + block] = this block's sum of r_j^2 (a
// vector's W squares first).  Every column: c_j = 0 (the next cycle's x = 0).  XV: x is read and written in W-wide vectors
// (the caller's x starts on a 16-byte boundary); the element operations and their bits are the same either way.
template <int W, bool XV>
__global__ __launch_bounds__(kThreads) void pcg_block_update_kernel(real* __restrict__ x, const real* __restrict__ u, real* __restrict__ r,
                                                                    real* __restrict__ c, int64_t n, int bs, const real* __restrict__ sc,
                                                                    const PbStatus* __restrict__ st, real* __restrict__ partial) {
  __shared__ real s_red[kThreads / kWave][kPbMaxCols];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t nv = n / W;
  for (int j = 0; j < bs; ++j) {
    PbVec<W>* cv = reinterpret_cast<PbVec<W>*>(c + j * n);
    PbVec<W> zero;
#pragma unroll
    for (int e = 0; e < W; ++e) zero.v[e] = 0.0;
    if (!st->active[j]) {
      for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nv; p += (int64_t)gridDim.x * blockDim.x) cv[p] = zero;
      continue;
    }
    const real ap = 1.0 * sc[kPbAlpha * kPbMaxCols + j], am = -1.0 * sc[kPbAlpha * kPbMaxCols + j];
    real* xj = x + j * n;
    const PbVec<W>* uv = reinterpret_cast<const PbVec<W>*>(u + j * n);
    PbVec<W>* rv = reinterpret_cast<PbVec<W>*>(r + j * n);
    real acc = 0.0;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nv; p += (int64_t)gridDim.x * blockDim.x) {
      const PbVec<W> ui = uv[p], ci = cv[p];
      PbVec<W> ri = rv[p];
      if constexpr (XV) {
        PbVec<W>* xv = reinterpret_cast<PbVec<W>*>(xj);
        PbVec<W> xi = xv[p];
#pragma unroll
        for (int e = 0; e < W; ++e) xi.v[e] = xi.v[e] + ap * ui.v[e];
        xv[p] = xi;
      } else {
#pragma unroll
        for (int e = 0; e < W; ++e) xj[p * W + e] = xj[p * W + e] + ap * ui.v[e];
      }
#pragma unroll
      for (int e = 0; e < W; ++e) ri.v[e] = ri.v[e] + am * ci.v[e];
      rv[p] = ri;
      cv[p] = zero;
      real s = ri.v[0] * ri.v[0];
#pragma unroll
      for (int e = 1; e < W; ++e) s += ri.v[e] * ri.v[e];
      acc += s;
    }
    const real t = pb_wave_sum(acc);
    if (lane == 0) s_red[wave][j] = t;
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < bs && st->active[j]) {
    real t = s_red[0][j];
    for (int q = 1; q < kThreads / kWave; ++q) t += s_red[q][j];
    partial[(int64_t)j * kRedBlocks + blockIdx.x] = t;
  }
}

}  // namespace amgh
