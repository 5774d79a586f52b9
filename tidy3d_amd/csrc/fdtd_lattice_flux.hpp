// The power through one surface of a projection monitor from its lattice accumulators (fdtd_lattice_dft.hpp), reduced on the device
// (ref tidy3d monitor.py DirectivityMonitor: directivity = 4 pi x radiation intensity / radiated power, the power being the flux
// of the time-averaged Poynting vector through the monitor's own surfaces).
//
// With the tangential axes a1 = axis + 1, a2 = axis + 2 (cyclic, so (a1, a2, axis) is right-handed whatever the axis and whatever
// cyclic renaming the caller applied) and the accumulators E_a1, E_a2, H_a1, H_a2 [nf][n2][n1][n0] of the surface,
//     out[k] = 0.5 sign  sum over the lattice nodes of  w0[i0] w1[i1] w2[i2] *
//              (Re E_a1 Re H_a2 + Im E_a1 Im H_a2 - Re E_a2 Re H_a1 - Im E_a2 Im H_a1)        = sign  int 0.5 Re(E x H*) . n dS
// in fp64: the fp32 accumulators are widened first, so each of the four products is exact, and only the sums round.  The weights
// are the trapezoid weights of the lattice along each axis ([1] along the normal), the ones the far-field integrals take.
//
// One workgroup of 256 threads per frequency and surface (a surface is one monitor of the C interface).  A thread strides over
// the nodes — node = t, t + 256, ... whatever the size of the lattice — and keeps one partial sum; the 64 lanes of a wave are
// folded by shuffles (offsets 32, 16, .. 1), the four wave sums go through LDS and thread 0 adds them in the order 0, 1, 2, 3.
// The order of every sum is fixed by the node index alone: no atomics, nothing depends on the launch shape.  Every thread of the
// workgroup reaches every shuffle and the barrier (no early exit).  Runs once, after the last step: it is no part of the time loop.
#pragma once
#include <hip/hip_runtime.h>

namespace fdtd {

constexpr int kLatticeFluxThreads = 256;

struct LatticeFluxP {
  const float2* acc;         // [nf][nodes]: the accumulators of the monitor (FieldDftP.acc)
  long long nodes;           // kept nodes of all four components (TapTables.nodes)
  long long off[4];          // where E_a1, E_a2, H_a1, H_a2 start inside a frequency
  int n[3];                  // lattice nodes along the axes (1 along the normal)
  const double* w[3];        // integration weights along the axes
  double half_sign;          // 0.5 x the orientation of the surface
  double* out;               // [nf]
};

__global__ __launch_bounds__(kLatticeFluxThreads) void lattice_flux_kernel(LatticeFluxP p) {
  const int k = (int)blockIdx.x;
  const int t = (int)threadIdx.x;
  const long long n0 = p.n[0], n01 = n0 * p.n[1], total = n01 * p.n[2];
  const float2* a = p.acc + (long long)k * p.nodes;
  double s = 0.0;
  for (long long i = t; i < total; i += kLatticeFluxThreads) {
    const long long r = i % n01;
    const double w = p.w[0][r % n0] * p.w[1][r / n0] * p.w[2][i / n01];
    const float2 e1 = a[p.off[0] + i], e2 = a[p.off[1] + i], h1 = a[p.off[2] + i], h2 = a[p.off[3] + i];
    const double v = (double)e1.x * (double)h2.x + (double)e1.y * (double)h2.y - (double)e2.x * (double)h1.x - (double)e2.y * (double)h1.y;
    s = s + w * v;
  }
  for (int d = 32; d > 0; d >>= 1) s = s + __shfl_down(s, (unsigned)d, 64);
  __shared__ double part[kLatticeFluxThreads / 64];
  if ((t & 63) == 0) part[t >> 6] = s;
  __syncthreads();
  if (t == 0) p.out[k] = p.half_sign * (((part[0] + part[1]) + part[2]) + part[3]);
}

}  // namespace fdtd
