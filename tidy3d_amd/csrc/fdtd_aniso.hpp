// Off-diagonal coupling of fully anisotropic bodies (ref tidy3d medium.py:5058 FullyAnisotropicMedium).
//
// The sweep advances every E component with the diagonal of eps^-1 (a table medium of permittivity 1 / [eps^-1]_aa); these three
// small gather kernels add, for the nodes inside such bodies,
//     dE_a(i) = sum_q  w_new[q] E_b^{n+1}(j_q) - w_old[q] E_b^n(j_q),      q = the four E_b nodes around i, b = the other two components
// with the host's weights  w_new = (dt / eps0) g(i, j) / Cb_b(j),  w_old = w_new Ca_b(j)  (tidy3d_amd/spec.py AnisoSet: g = the
// symmetric average of [eps^-1]_ab over both nodes / 4; (E^{n+1} - Ca E^n) / Cb is the curl the sweep applied at j).
// E^n of the neighbours is saved in front of the sweep (the two-pass kernels update E in place), the corrections of all three
// components are formed from the UNPATCHED new values and applied afterwards.  Lists, not planes: these bodies are small.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fdtd {

constexpr uint32_t kNoNode = 0xFFFFFFFFu;

// old[q] = E_b^n(nbr[q]); slot q % 8 < 4 -> component b1, else b2
__global__ __launch_bounds__(256) void aniso_save_kernel(const float* __restrict__ eb1, const float* __restrict__ eb2,
                                                         const uint32_t* __restrict__ nbr, float* __restrict__ old, long long n8) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n8) return;
  const uint32_t j = nbr[q];
  const float* src = (q & 7) < 4 ? eb1 : eb2;
  old[q] = j != kNoNode ? src[j] : 0.0f;
}

__global__ __launch_bounds__(256) void aniso_delta_kernel(const float* __restrict__ eb1, const float* __restrict__ eb2,
                                                          const uint32_t* __restrict__ nbr, const float* __restrict__ w_new,
                                                          const float* __restrict__ w_old, const float* __restrict__ old,
                                                          float* __restrict__ delta, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float d = 0.0f;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const long long q = i * 8 + s;
    const uint32_t j = nbr[q];
    if (j == kNoNode) continue;
    const float en = (s < 4 ? eb1 : eb2)[j];
    d += w_new[q] * en - w_old[q] * old[q];
  }
  delta[i] = d;
}

// Bloch form (fdtd_run_bloch): the Re and Im solvers carry the same lists.  A neighbour slot one period away across a Bloch face
// holds the real node on the far side and a wrap code, the sign of the period crossed on each axis a in bits 2a, 2a+1 (0 = none,
// 1 = +1, 2 = -1); that node stands for exp(i sum_a s_a phi_a) E(j), so its term mixes the two parts.  The row reached from the
// other side crosses with the opposite signs and gets the conjugate factor: the coupling stays Hermitian.  Code 0 = no rotation.
constexpr int kWrapCodes = 64;
struct AnisoPhaseTab {
  float2 r[kWrapCodes];            // (cos, sin) of the phase of each wrap code
};

// E^n of both parts (rotated with the new values in the delta kernel: the phase factor is linear)
__global__ __launch_bounds__(256) void aniso_save_bloch_kernel(const float* __restrict__ eb1_re, const float* __restrict__ eb2_re,
                                                               const float* __restrict__ eb1_im, const float* __restrict__ eb2_im,
                                                               const uint32_t* __restrict__ nbr, float* __restrict__ old_re,
                                                               float* __restrict__ old_im, long long n8) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n8) return;
  const uint32_t j = nbr[q];
  const bool b1 = (q & 7) < 4;
  old_re[q] = j != kNoNode ? (b1 ? eb1_re : eb2_re)[j] : 0.0f;
  old_im[q] = j != kNoNode ? (b1 ? eb1_im : eb2_im)[j] : 0.0f;
}

// the deltas of both parts of every row from both parts' fields; wrap = nullptr: no slot crosses a Bloch face
__global__ __launch_bounds__(256) void aniso_delta_bloch_kernel(const float* __restrict__ eb1_re, const float* __restrict__ eb2_re,
                                                                const float* __restrict__ eb1_im, const float* __restrict__ eb2_im,
                                                                const uint32_t* __restrict__ nbr, const uint8_t* __restrict__ wrap,
                                                                const float* __restrict__ w_new, const float* __restrict__ w_old,
                                                                const float* __restrict__ old_re, const float* __restrict__ old_im,
                                                                AnisoPhaseTab tab, float* __restrict__ delta_re,
                                                                float* __restrict__ delta_im, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float dr = 0.0f, di = 0.0f;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const long long q = i * 8 + s;
    const uint32_t j = nbr[q];
    if (j == kNoNode) continue;
    const float xr = w_new[q] * (s < 4 ? eb1_re : eb2_re)[j] - w_old[q] * old_re[q];
    const float xi = w_new[q] * (s < 4 ? eb1_im : eb2_im)[j] - w_old[q] * old_im[q];
    const int c = wrap ? wrap[q] : 0;
    if (c == 0) {
      dr += xr;
      di += xi;
    } else {
      const float2 p = tab.r[c];
      dr += p.x * xr - p.y * xi;
      di += p.y * xr + p.x * xi;
    }
  }
  delta_re[i] = dr;
  delta_im[i] = di;
}

__global__ __launch_bounds__(256) void aniso_apply_kernel(float* __restrict__ ea, const uint32_t* __restrict__ cell,
                                                          const float* __restrict__ delta, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ea[cell[i]] += delta[i];
}

}  // namespace fdtd
