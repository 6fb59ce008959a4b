// dist_pcg_kernels.hpp — gfx950 kernels of the device-resident PCG on a row-sharded hierarchy (amgh_dist_pcg_d,
// amghip_dist.hpp).
//
// The recurrence is pcg_dev's (IterativeSolvers.jl's cg, x0 = 0) on this rank's rows; the scalars of an iteration are sums
// over ALL ranks, so they pass through the host: a rank's partial sum is read back, all-reduced in double, and alpha / beta
// come back into the next kernel as ARGUMENTS (host doubles, the same bits on every rank) — where pcg_dev keeps them on
// the device.  Between the cycle and the sharded SpMV an iteration is at most four passes over the local rows:
//   dot_partial_kernel   partial[b] = block b's sum of z_i r_i          (rho'; preconditioned only: plain CG has rho' = |r|^2)
//   dpcg_dir_kernel      u = z + beta u                                 (z = r for plain CG)
//   [sharded SpMV        c = A u, halo of u exchanged in front]
//   dot_partial_kernel   partial[b] = block b's sum of u_i c_i          (the stream kernel's epilogue is shared by every mode
//                                                                        of every operator: the dot stays a pass of its own)
//   dpcg_update_kernel   x += alpha u, r -= alpha c, partial[b] = block b's sum of r_i^2  — three passes and a norm in one
// Memory-bound wave64 kernels, grid-stride; every sum is per-block partials in block order over a row partition that depends
// on n only, finished by reduce_final_kernel in a fixed order (no atomics): a run is bitwise reproducible.
#pragma once
#include "amghip_kernels.hpp"

namespace amgh {

// u = c + beta u  (c: the cycle's result in the level's x, or r itself)
__global__ __launch_bounds__(kThreads) void dpcg_dir_kernel(real* __restrict__ u, const real* __restrict__ c, double beta, int64_t n) {
  const real be = (real)beta;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) u[i] = c[i] + be * u[i];
}

// x += alpha u, r -= alpha c, partial[blockIdx.x] = this block's sum of the new r_i^2 (pcg_update_kernel's arithmetic)
__global__ __launch_bounds__(kThreads) void dpcg_update_kernel(real* __restrict__ x, const real* __restrict__ u, real* __restrict__ r,
                                                                 const real* __restrict__ c, double alpha, int64_t n,
                                                                 real* __restrict__ partial) {
  __shared__ real s_part[kThreads / kWave];
  const real ap = (real)alpha, am = -(real)alpha;
  real v = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    x[i] = x[i] + ap * u[i];
    const real rn = r[i] + am * c[i];
    r[i] = rn;
    v += rn * rn;
  }
  const real t = block_reduce_sum(v, s_part);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

}  // namespace amgh
