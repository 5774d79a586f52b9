// PEC-conformal boundaries (ref tidy3d components/subpixel_spec.py PECConformal; the Dey-Mittra conformal scheme).
//
// A face of the primal grid cut by a PEC surface is advanced with
//     H_c^{n+1/2} = H_c^{n-1/2} - (dt / mu0) / (A S) sum_k s_k l_k L_k E_k^n,      k = its four edges
// (l_k: the free fraction of edge k, A: the free fraction of the face's area, clamped from below by the host).  The sweep applies the
// same sum with l_k / A = 1, so for the listed faces one small gather kernel adds, in FRONT of the sweep (h_side_terms: the correction
// reads E^n alone),
//     H_c += sum_k d[k] E_k^n,      d[k] = -(dt / mu0) s_k (l_k / A - 1) * inv_step_k
// with the float32 inverse step the sweep itself reads for that difference.  Slots: a1 = (c + 1) % 3, a2 = (c + 2) % 3; k = 0, 1: E_a2
// one node up along a1 / at the face's own index, k = 2, 3: E_a1 one node up along a2 / at the face's own index.  A slot without a node
// (a PEC edge, an edge beyond a wall) holds kNoNode.  One thread per face, a fixed summation order k = 0..3, one read-modify-write of
// H, no atomics: a face appears once per list.  Structure of arrays: nbr and d are [4][n], lane i reads entry i of every row.
// Single steps only (FDTD_F2_OFF_CONFORMAL); one GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "fdtd_aniso.hpp"          // kNoNode

namespace fdtd {

__global__ __launch_bounds__(256) void conformal_h_kernel(float* __restrict__ hc, const float* __restrict__ e_a2,
                                                          const float* __restrict__ e_a1, const uint32_t* __restrict__ cell,
                                                          const uint32_t* __restrict__ nbr, const float* __restrict__ d, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t j = nbr[(long long)k * n + i];
    if (j == kNoNode) continue;
    acc += d[(long long)k * n + i] * (k < 2 ? e_a2 : e_a1)[j];
  }
  hc[cell[i]] += acc;
}

}  // namespace fdtd
