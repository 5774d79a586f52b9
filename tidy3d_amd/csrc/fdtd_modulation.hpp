// Time-modulated media (ref tidy3d components/time_modulation.py ModulationSpec: SpaceTimeModulation = SpaceModulation x
// ContinuousWaveTimeModulation on Medium.permittivity and / or Medium.conductivity).
//
//     eps(r, t)   = eps_bar(r)   + Re[ d_eps(r) exp(-i w_eps t) ]
//     sigma(r, t) = sigma_bar(r) + Re[ d_sig(r) exp(-i w_sig t) ]          (the time modulation's amplitude and phase folded into d)
//
// The sweep and everything behind it (CPML, sources, TFSF corrections, ADE) advance every node with its STATIC table medium:
// E_lin = Ca E^n + Cb K.  For the listed nodes two small list kernels turn that into the update of
//     (D^{n+1} - D^n) / dt + sigma^{n+1/2} (E^{n+1} + E^n) / 2 = K,      D = eps0 eps(t) E:
//     E^{n+1} = alpha E^n + beta (E_lin - Ca E^n)
//     alpha = (eps^n - s) / (eps^{n+1} + s),   beta = (eps_bar + s_bar) / (eps^{n+1} + s),   s = sigma^{n+1/2} dt / (2 eps0)
// with eps_bar = dt / (eps0 Cb) * 2 / (1 + Ca), s_bar = eps_bar (1 - Ca) / (1 + Ca) recovered by the host from the node's own table
// entry (sub-pixel value included): Cb = dt / (eps0 (eps_bar + s_bar)), so beta (E_lin - Ca E^n) = K dt / (eps0 (eps^{n+1} + s)).
// With d_eps = d_s = 0: alpha = Ca, beta = 1 — the table update.  E^n is saved in front of the sweep (the two-pass kernels update E
// in place).  The host passes (cos, sin) of w_eps n dt, w_eps (n + 1) dt and w_sig (n + 1/2) dt, formed in double: no transcendental
// per node.  Structure of arrays: lane i reads entry i of every array.  Single steps only (FDTD_F2_OFF_MODULATION); one GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fdtd {

struct ModPhase {                  // Re[d exp(-i th)] = d.x cos th + d.y sin th
  float c0, s0;                    // th = w_eps n dt
  float c1, s1;                    // th = w_eps (n + 1) dt
  float ch, sh;                    // th = w_sig (n + 1/2) dt
};

// old[i] = E^n(cell[i])
__global__ __launch_bounds__(256) void modulation_save_kernel(const float* __restrict__ e, const uint32_t* __restrict__ cell,
                                                              float* __restrict__ old, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) old[i] = e[cell[i]];
}

__global__ __launch_bounds__(256) void modulation_apply_kernel(float* __restrict__ e, const uint32_t* __restrict__ cell,
                                                               const float* __restrict__ ca, const float* __restrict__ eps_bar,
                                                               const float* __restrict__ s_bar, const float2* __restrict__ d_eps,
                                                               const float2* __restrict__ d_s, const float* __restrict__ old,
                                                               ModPhase p, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = cell[i];
  const float eb = eps_bar[i], sb = s_bar[i], e_old = old[i];
  const float2 de = d_eps[i], ds = d_s[i];
  const float eps_n = eb + (de.x * p.c0 + de.y * p.s0);
  const float eps_n1 = eb + (de.x * p.c1 + de.y * p.s1);
  const float s = sb + (ds.x * p.ch + ds.y * p.sh);
  const float inv = 1.0f / (eps_n1 + s);
  const float alpha = (eps_n - s) * inv, beta = (eb + sb) * inv;
  e[j] = alpha * e_old + beta * (e[j] - ca[i] * e_old);
}

}  // namespace fdtd
