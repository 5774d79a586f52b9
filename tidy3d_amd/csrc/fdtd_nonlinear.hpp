// Kerr media (ref tidy3d components/medium.py NonlinearSpec with NonlinearSusceptibility models): the instantaneous third-order
// response  D = eps0 (eps_bar + chi3 I) E,  I = |E|^2 at the node.
//
// The sweep and everything behind it (CPML, sources, TFSF corrections, damping, ADE) advance every node with its STATIC table
// medium: E_lin = Ca E^n + Cb K.  For the listed nodes the library solves
//     (D^{n+1} - D^n) / dt + sigma (E^{n+1} + E^n) / 2 = K
// by num_iters Jacobi fixed-point iterations, E^(0) = E_lin,
//     E^(m) = alpha_m E^n + beta_m (E_lin - Ca E^n)
//     alpha_m = (eps_bar + chi3 I^n - s_bar) / (eps_bar + chi3 I^(m-1) + s_bar),   beta_m = (eps_bar + s_bar) / (eps_bar + chi3 I^(m-1) + s_bar)
// with eps_bar, s_bar recovered by the host from the node's own table entry (fdtd_modulation.hpp).  Because Ca = (eps_bar - s_bar) /
// (eps_bar + s_bar), alpha_m - beta_m Ca = chi3 I^n / den and beta_m - 1 = -chi3 I^(m-1) / den: the kernel evaluates the same iterate as
//     E^(m) = E_lin + chi3 (I^n E^n - I^(m-1) E_lin) / (eps_bar + s_bar + chi3 I^(m-1))
// — a correction to E_lin that is exactly zero with chi3 = 0 (the table update, bit for bit) and needs neither Ca nor a difference of
// two nearly equal products.
//
// Intensity at a node of component a:  I = E_a^2 + (mean of the four surrounding E_b nodes)^2 + (mean of the four surrounding E_c
// nodes)^2, b = a + 1, c = a + 2 (cyclic); the eight slots have the layout of the fully anisotropic lists (spec.AnisoSet.nbr_ijk:
// slots 0..3 component b, 4..7 component c; periodic faces wrap); a slot without a node (kNoNode: beyond a PEC / PMC wall)
// contributes 0 to its mean of four.
//
// Three list kernels, one node per lane, structure of arrays (nbr is [8][n]), blockIdx.y = component — one launch covers the lists of
// all three components:
//   nonlinear_save_kernel     in front of the sweep:  old = E^n, i_old = I^n
//   nonlinear_iter_kernel     next = E^(m) from the fields as iteration m - 1 left them (the first one keeps E_lin in `lin`)
//   nonlinear_scatter_kernel  E = next
// Jacobi: every listed node of all three components is computed before any is overwritten (all computes, then all scatters): the
// result does not depend on list or launch order.  No atomics, no transcendental functions.  Single steps only
// (FDTD_F2_OFF_NONLINEAR); one GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "fdtd_aniso.hpp"          // kNoNode

namespace fdtd {

struct NonlinearList {             // the listed nodes of one E component (n = 0: none)
  const uint32_t* cell;            // [n]
  const uint32_t* nbr;             // [8][n]
  const float* den0;               // [n] eps_bar + s_bar
  const float* chi3;               // [n]
  float* old;                      // [n] E^n
  float* i_old;                    // [n] I^n
  float* lin;                      // [n] E_lin
  float* next;                     // [n] the iterate being formed
  long long n;
};
struct NonlinearP {
  NonlinearList l[3];
  float* e[3];                     // the current E arrays
};

__device__ __forceinline__ float nonlinear_intensity(float ea, const float* __restrict__ eb, const float* __restrict__ ec,
                                                     const uint32_t* __restrict__ nbr, long long n, long long i) {
  float sb = 0.0f, sc = 0.0f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const uint32_t j = nbr[(long long)s * n + i];
    sb += j != kNoNode ? eb[j] : 0.0f;
  }
#pragma unroll
  for (int s = 4; s < 8; ++s) {
    const uint32_t j = nbr[(long long)s * n + i];
    sc += j != kNoNode ? ec[j] : 0.0f;
  }
  const float mb = 0.25f * sb, mc = 0.25f * sc;
  return ea * ea + mb * mb + mc * mc;
}

__global__ __launch_bounds__(256) void nonlinear_save_kernel(NonlinearP p) {
  const int a = blockIdx.y;
  const NonlinearList& L = p.l[a];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  const float ea = p.e[a][L.cell[i]];
  L.old[i] = ea;
  L.i_old[i] = nonlinear_intensity(ea, p.e[(a + 1) % 3], p.e[(a + 2) % 3], L.nbr, L.n, i);
}

// first != 0: iteration 1 — the field array holds E^(0) = E_lin, kept in `lin` for the iterations behind it
__global__ __launch_bounds__(256) void nonlinear_iter_kernel(NonlinearP p, int first) {
  const int a = blockIdx.y;
  const NonlinearList& L = p.l[a];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  const float ea = p.e[a][L.cell[i]];
  const float e_lin = first ? ea : L.lin[i];
  if (first) L.lin[i] = ea;
  const float in = nonlinear_intensity(ea, p.e[(a + 1) % 3], p.e[(a + 2) % 3], L.nbr, L.n, i);
  const float c3 = L.chi3[i];
  const float den = L.den0[i] + c3 * in;
  L.next[i] = e_lin + c3 * (L.i_old[i] * L.old[i] - in * e_lin) / den;
}

__global__ __launch_bounds__(256) void nonlinear_scatter_kernel(NonlinearP p) {
  const int a = blockIdx.y;
  const NonlinearList& L = p.l[a];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L.n) p.e[a][L.cell[i]] = L.next[i];
}

}  // namespace fdtd
